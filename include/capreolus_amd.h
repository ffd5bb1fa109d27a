/*
 * capreolus_amd.h — C ABI of the MI355X (gfx950) reranker scoring engine.
 *
 * Drop-in boundary for the inference forward pass of three Capreolus rerankers.  The reference
 * has no FFI (it is pure Python); each entry point below names the reference
 * Python interface it replaces (file:line under the reference tree) and is what a ctypes stub
 * on the reference side binds (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host; the library allocates
 *     nothing and frees nothing; the caller (the PyTorch caching allocator) owns inputs, outputs
 *     and workspaces.
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); kernels are
 *     enqueued and the call returns without synchronising (reference sync point:
 *     capreolus/trainer/pytorch.py:345).
 *   - return value: CAPAMD_OK or a CAPAMD_ERR_* (argument / launch errors, never an exception,
 *     never abort()).  Data-dependent errors (an id >= V, ...) are reported asynchronously by
 *     OR-ing CAPAMD_STATUS_* bits into the caller-zeroed int32 `status` word in device memory;
 *     the offending term is scored as a pad so the launch itself never faults.
 *   - ids are int64 exactly as the extractors emit them (embedtext.py:146-147,
 *     bertpassage.py:308-310): 0 = pad, negative = OOV term.
 */
#ifndef CAPREOLUS_AMD_H
#define CAPREOLUS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAPAMD_VERSION 405   /* (the DeepTileBar entries below were added without a new number: purely additive, nothing existing changed) */

#define CAPAMD_OK 0
#define CAPAMD_ERR_ARG 1       /* null pointer / bad size / unsupported configuration */
#define CAPAMD_ERR_ALIGN 2     /* pointer not aligned as documented */
#define CAPAMD_ERR_LAUNCH 3    /* hipLaunchKernel reported an error */
#define CAPAMD_ERR_WORKSPACE 4 /* workspace too small */

#define CAPAMD_STATUS_DOC_ID_RANGE 1   /* a document term id >= V        (torch raises IndexError) */
#define CAPAMD_STATUS_QUERY_ID_RANGE 2 /* a query term id >= V */
#define CAPAMD_STATUS_QUERY_OOV 4      /* negative query id in DRMM      (reference DRMM.py:109 raises IndexError) */
#define CAPAMD_STATUS_SCORE_NAN 8      /* a NaN score reached the ranking kernels (ranked last) */
#define CAPAMD_STATUS_TIE_RANGE 16     /* capamd_ndcg_cut: a tie-break rank outside 0..n-1 */
#define CAPAMD_STATUS_LIST_QUERY 32    /* *_forward_lists: a pair of a list brings another query row (DRMM, DRMM-TKS: or another idf row) than
                                          the list's first pair - a list is ONE query against its documents */
#define CAPAMD_STATUS_SHORT_DOC 64     /* capamd_posit_forward: a document of fewer than 2 non-pad terms (the reference divides by zero) */
#define CAPAMD_STATUS_SEGMENT_RANGE 128 /* capamd_deeptile_color: a segment offset decreases or leaves [0, L] (clamped; nothing is read outside the row) */
#define CAPAMD_STATUS_BAG_RANGE 256     /* capamd_dssm_tower: an indptr pair decreases or leaves [0, nnz] (clamped; nothing is read outside idx / val) */

/* library identity */
int capamd_version(void);
const char* capamd_arch(void); /* "gfx950" */

/* Per-call launch flags of the interaction scoring entries (`flags` argument; no process-wide state).
 * CAPAMD_LAUNCH_CONCURRENT: the caller keeps several scoring calls in flight on different streams (one candidate list per launch,
 * the reference's PytorchTrainer.predict loop at small evalbatch, trainer/pytorch.py:334-348), so a small launch no longer has the
 * chip to itself: the kernels then use their occupancy-oriented variant at every batch size instead of the latency-oriented one
 * they pick for a lone launch of <= 1536 pairs.  Scores are bit-identical either way. */
#define CAPAMD_LAUNCH_CONCURRENT 1u

/* Workspace of the interaction scoring entries (`workspace`, `workspace_bytes`): a few bytes of device memory the caller owns (any
 * contents; 4-byte aligned; one per call in flight).  Launches that outnumber the workgroups the chip holds run persistent
 * workgroups that draw their pairs from a ticket counter kept there (zeroed by the call, on `stream`).  NULL / too small: allowed,
 * every launch then runs one workgroup per pair.  Scores do not depend on it beyond the last bits of fp32 rounding. */
size_t capamd_interaction_workspace_bytes(void);

/* ---- embedding table ------------------------------------------------------------------------
 * Replaces create_emb_layer + nn.Embedding lookup (capreolus/reranker/common.py:279-288, :161).
 * The fp32 [V, D] table (row 0 = zeros, extractor/common.py:38-40) is re-laid out once into
 * rows of capamd_packed_row_stride(D) floats (256-byte aligned rows, |row|+1e-9 in the last
 * float); all forward calls take the packed table.  D <= 319. */
int64_t capamd_packed_row_stride(int D);               /* floats per packed row, -1 if unsupported */
int64_t capamd_packed_table_bytes(int64_t V, int D);   /* bytes the caller must allocate (256-B aligned) */
int capamd_pack_embeddings(const float* emb, int64_t V, int D, int64_t ld /* floats between rows of emb */,
                           float* packed, void* stream);

/* ---- SimilarityMatrix.forward (capreolus/reranker/common.py:170-182) ------------------------
 * sim_out fp32 [B, Q, L] = exact-match(OOV) + cosine(in-vocab), pads zeroed. */
int capamd_similarity_matrix(const int64_t* q_ids /*[B,Q]*/, const int64_t* d_ids /*[B,L]*/, int B, int Q, int L,
                             const float* packed, int64_t V, int D, float* sim_out, int* status, void* stream);

/* ---- KNRM_class.forward (capreolus/reranker/KNRM.py:39-55) behind KNRM.test (KNRM.py:96-101) --
 * mu, sigma: fp32 [K] (RbfKernel parameters, common.py:229-230; K <= 12, reference K = 11).
 * combine (KNRM.py:27-34): hidden == 0 -> score = w1[0,:K]·f + b1[0]            ("singlefc")
 *                          hidden  > 0 -> score = w2[0,:hidden]·tanh(w1·f + b1) + b2[0]
 *                          scoretanh != 0 applies a final tanh.
 * out fp32 [B].  workspace / flags: see CAPAMD_LAUNCH_* and capamd_interaction_workspace_bytes above.
 * L: the document's term list lives in LDS (8 bytes per position beside ~11 KiB of fixed parts): documents beyond ~19,000 positions
 * do not fit the 160 KiB of a workgroup and are refused with CAPAMD_ERR_ARG (DRMM alike). */
int capamd_knrm_forward(const int64_t* q_ids /*[B,Q]*/, const int64_t* d_ids /*[B,L]*/, int B, int Q, int L,
                        const float* packed, int64_t V, int D, const float* mu, const float* sigma, int K,
                        const float* w1, const float* b1, int hidden, const float* w2, const float* b2, int scoretanh,
                        float* out, int* status, void* workspace, size_t workspace_bytes, unsigned flags, void* stream);

/* Forward half of the training step (reference trainer/pytorch.py:96-99 -> KNRM.score):
 * the kernel-pooling features f[b][k] = sum_q mask_q log(sum_j K_k(sim_qj) + 1e-6) (KNRM.py:50-53) that feed `combine`,
 * and their derivatives w.r.t. the RbfKernel parameters (trainable when `gradkernels`).  The embedding is frozen
 * (`finetune = False`, KNRM.py:23); `combine` and the loss run under autograd on these [B, K] tensors.
 * dfdmu_out / dfdsigma_out may be NULL. */
int capamd_knrm_features(const int64_t* q_ids, const int64_t* d_ids, int B, int Q, int L, const float* packed, int64_t V,
                         int D, const float* mu, const float* sigma, int K, float* feat_out, float* dfdmu_out,
                         float* dfdsigma_out, int* status, void* stream);

/* One KNRM training step on the device, no host round trip (reference capreolus/trainer/pytorch.py:93-108):
 * `reranker.score()` on B (query, positive document, negative document) triples -> the trainer's pairwise loss (loss_type 0: hinge,
 * reranker/common.py:101-103; 1: softmax, :96-98) -> backward through `combine` (a single Linear, KNRM.py:27-34: `singlefc`; under tanh when
 * `scoretanh`) and the RBF kernels' mu / sigma (when train_kernels: `gradkernels`) -> torch.optim.Adam's in-place update (betas / eps as
 * given, no weight decay, no amsgrad).  The caller owns the step count and hands in what depends on it, computed in double as the plain
 * Adam of the reference does: step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t).
 * ptrs: DEVICE array of 3 P device pointers, P = 2 K + 2 - the parameters (mu_0 .. mu_{K-1}, sigma_0 .. sigma_{K-1}: one scalar each, as the
 * reference's state_dict names them, common.py:229-230; the Linear's weight [K]; its bias [1]), then their exp_avg, then their exp_avg_sq
 * (the mu / sigma moments may be NULL when !train_kernels).  loss_out: [1] the batch's mean loss.  workspace:
 * capamd_knrm_train_step_workspace_floats(B, K) floats.  B <= 1024.  Two launches on `stream`: capamd_knrm_features' kernel over the 2 B
 * documents (it reads the scalar kernel parameters through `ptrs`), then one workgroup for everything that is per batch. */
size_t capamd_knrm_train_step_workspace_floats(int B, int K);
int capamd_knrm_train_step(const int64_t* q_ids, const int64_t* pos_ids, const int64_t* neg_ids, int B, int Q, int L, const float* packed,
                           int64_t V, int D, int K, float* const* ptrs, int train_kernels, int scoretanh, int loss_type, float step_size,
                           float one_minus_beta1, float beta2, float eps, float bc2_sqrt, float* loss_out, float* workspace,
                           size_t workspace_floats, int* status, void* stream);

/* Same scoring from a device-resident candidate store (replaces the per-sample
 * PredSampler -> DataLoader collate -> .to(device) of capreolus/sampler/__init__.py:207-264 and
 * trainer/pytorch.py:334-342): the run's query / document id rows are uploaded ONCE as int32 tables
 * q_table [NQ, Q], d_table [ND, L]; a batch is B (query row, document row) index pairs. */
int capamd_knrm_forward_indexed(const int32_t* q_table, const int32_t* d_table, const int32_t* pair_q,
                                const int32_t* pair_d, int B, int Q, int L, const float* packed, int64_t V, int D,
                                const float* mu, const float* sigma, int K, const float* w1, const float* b1, int hidden,
                                const float* w2, const float* b2, int scoretanh, float* out, int* status, void* workspace,
                                size_t workspace_bytes, unsigned flags, void* stream);

/* ---- DRMM_class.forward (capreolus/reranker/DRMM.py:101-116) behind DRMM.test (DRMM.py:150-155)
 * idf fp32 [B,Q]; edges fp32 [nbins] = torch.linspace(-1,1,nbins+1)[1:] (DRMM.py:63);
 * hist_type 0 = CH, 1 = NH, 2 = LCH (DRMM.py:72-79); gate_type 0 = IDF (gate_w fp32 [1]),
 * 1 = TV (gate_w fp32 [D], emb_raw = the un-packed fp32 [V, D] table with leading dim ld);
 * ffw: w1 [nodes, nbins+1], b1 [nodes], w2 [nodes], b2 [1]; out_w [1], out_b [1].
 * nbins <= 63, nodes <= 64, Q <= 32.  counts_out: optional int32 [B, Q, nbins+1] raw bin counts
 * (may be NULL).  out fp32 [B]. */
int capamd_drmm_forward(const int64_t* q_ids, const int64_t* d_ids, const float* idf, int B, int Q, int L,
                        const float* packed, int64_t V, int D, const float* edges, int nbins, int hist_type,
                        int gate_type, const float* gate_w, const float* emb_raw, int64_t ld, const float* w1,
                        const float* b1, int nodes, const float* w2, const float* b2, const float* out_w,
                        const float* out_b, float* out, int32_t* counts_out, int* status, void* workspace, size_t workspace_bytes,
                        unsigned flags, void* stream);

/* Training-step forward half for DRMM: feat_out fp32 [B, Q, nbins+1] = the matching histogram after CH/NH/LCH
 * (DRMM._hist_map, DRMM.py:41-81; it has no trainable inputs, the embedding is frozen at DRMM.py:22); the
 * feed-forward net, gate and output layer run under autograd on it. */
int capamd_drmm_features(const int64_t* q_ids, const int64_t* d_ids, int B, int Q, int L, const float* packed, int64_t V,
                         int D, const float* edges, int nbins, int hist_type, float* feat_out, int* status, void* stream);

/* One DRMM training step on the device (see capamd_knrm_train_step; reference DRMM.py:101-116 under trainer/pytorch.py:93-108; gateType = IDF):
 * matching histograms of the 2 B documents, the 30 -> nodes -> 1 tanh net per query term, softmax idf gate, output layer, the pairwise loss
 * (0 hinge / 1 softmax), backward and torch.optim.Adam's in-place update, in two launches.  ptrs: DEVICE array of 3 x 7 device pointers -
 * ffw.0.weight [nodes, nbins + 1], ffw.0.bias [nodes], ffw.2.weight [nodes], ffw.2.bias [1], gates.weight [1], output_layer.weight [1],
 * output_layer.bias [1], then their exp_avg, then their exp_avg_sq.  idf: [B, Q].  workspace:
 * capamd_drmm_train_step_workspace_floats(B, Q, nbins, nodes) floats.  B <= 1024, nodes <= 16. */
size_t capamd_drmm_train_step_workspace_floats(int B, int Q, int nbins, int nodes);
int capamd_drmm_train_step(const int64_t* q_ids, const int64_t* pos_ids, const int64_t* neg_ids, const float* idf, int B, int Q, int L,
                           const float* packed, int64_t V, int D, const float* edges, int nbins, int hist_type, int nodes, float* const* ptrs,
                           int loss_type, float step_size, float one_minus_beta1, float beta2, float eps, float bc2_sqrt, float* loss_out,
                           float* workspace, size_t workspace_floats, int* status, void* stream);

/* indexed variant (see capamd_knrm_forward_indexed); idf_table fp32 [NQ, Q] is indexed by the pair's query row */
int capamd_drmm_forward_indexed(const int32_t* q_table, const int32_t* d_table, const float* idf_table,
                                const int32_t* pair_q, const int32_t* pair_d, int B, int Q, int L, const float* packed,
                                int64_t V, int D, const float* edges, int nbins, int hist_type, int gate_type,
                                const float* gate_w, const float* emb_raw, int64_t ld, const float* w1, const float* b1,
                                int nodes, const float* w2, const float* b2, const float* out_w, const float* out_b,
                                float* out, int32_t* counts_out, int* status, void* workspace, size_t workspace_bytes, unsigned flags,
                                void* stream);

/* ---- KNRM / DRMM over whole candidate lists (what PytorchTrainer.predict scores: one query, its first-stage documents;
 * capreolus/trainer/pytorch.py:310-353 over PredSampler's per-query lists, sampler/__init__.py:222-233) ------------------------
 * The similarity of a document term to the query depends on (query, term) only, and the documents of a list share their vocabulary:
 * per list every distinct term's packed row is gathered ONCE (same arithmetic as the per-pair entries: bit-identical similarities)
 * into a float4 table over the vocabulary, and every document is pooled from 16-byte lookups.  DRMM's scores are bit-identical to
 * capamd_drmm_forward's, KNRM's equal to fp32 rounding of the pooling sums (another summation order).
 * Pairs are laid out list after list: list l owns pairs list_offsets_host[l] .. list_offsets_host[l+1] (a HOST array of n_lists + 1
 * entries) and is scored against the query of its FIRST pair (and, DRMM, that pair's idf row); a pair whose own query (idf) row differs
 * sets CAPAMD_STATUS_LIST_QUERY - the scores of such a call are those of the first pair's query, not the reference's.  Ids either as [B,Q] / [B,L] int64
 * (q_ids, d_ids; the table arguments NULL) or through a candidate store (q_table, d_table, pair_q, pair_d; q_ids / d_ids NULL).
 * Q <= 8 (two blocks of four query terms; the reference's `maxqlen` is a free ConfigOption, extractor/embedtext.py:28-31, its forwards
 * take any Q: reranker/KNRM.py:39-55, DRMM.py:101-116; capamd_pacrr_forward_lists: Q <= 4); the other limits as the per-pair entries.
 * workspace: capamd_lists_workspace_bytes_q(n_lists, V, n_pairs, L, Q) bytes (16-byte aligned; any contents;
 * capamd_lists_workspace_bytes(...) = the same for Q <= 4), in two parts:
 *   per PAIR of the call   4 x L + 48 bytes: the document's real term ids, compacted to int32 by the first pass (what the pooling pass reads
 *                          instead of the [L] id row), and its pad / OOV counts - 3.2 KB per pair at L = 800 (capamd_pacrr_forward_lists keeps
 *                          416 B of features per pair there and runs its combine layers in one pass behind the convolutions; with n_pairs = 0
 *                          - no such room - every pair's combine layers run inside its convolution workgroup: same scores, slower)
 *   per LIST in flight     17 B x V + 5 KB (a 16-byte table entry and a flag byte per vocabulary id): 6.8 MB at V = 400,001, 68 MB at V = 4 M
 *                          (queries of five to eight terms: a second 16-byte entry per id and a second 5 KB: 33 B x V + 10 KB);
 *                          at most 256 lists are in flight at a time - FEWER when the buffer is smaller (a caller bounds the workspace by
 *                          handing in less: the lists are then processed in more, smaller groups; CAPAMD_ERR_WORKSPACE below one list). */
size_t capamd_lists_workspace_bytes(int n_lists, int64_t V, int64_t n_pairs, int L);
size_t capamd_lists_workspace_bytes_q(int n_lists, int64_t V, int64_t n_pairs, int L, int Q);
int capamd_knrm_forward_lists(const int64_t* q_ids, const int64_t* d_ids, const int32_t* q_table, const int32_t* d_table, const int32_t* pair_q,
                              const int32_t* pair_d, const int64_t* list_offsets_host, int n_lists, int Q, int L, const float* packed, int64_t V,
                              int D, const float* mu, const float* sigma, int K, const float* w1, const float* b1, int hidden, const float* w2,
                              const float* b2, int scoretanh, float* out, int* status, void* workspace, size_t workspace_bytes, void* stream);
int capamd_drmm_forward_lists(const int64_t* q_ids, const int64_t* d_ids, const int32_t* q_table, const int32_t* d_table, const int32_t* pair_q,
                              const int32_t* pair_d, const float* idf, const int64_t* list_offsets_host, int n_lists, int Q, int L,
                              const float* packed, int64_t V, int D, const float* edges, int nbins, int hist_type, int gate_type,
                              const float* gate_w, const float* emb_raw, int64_t ld, const float* w1, const float* b1, int nodes, const float* w2,
                              const float* b2, const float* out_w, const float* out_b, float* out, int32_t* counts_out, int* status,
                              void* workspace, size_t workspace_bytes, void* stream);
/* DRMM-TKS the same way (the float form of the table, then per document the top-k of every query term's lookups): scores bit-identical
 * to capamd_drmmtks_forward's (selections of bit-identical similarities, fed to the Linear in the same order).  IDF gate; Q <= 4. */
int capamd_drmmtks_forward_lists(const int64_t* q_ids, const int64_t* d_ids, const int32_t* q_table, const int32_t* d_table, const int32_t* pair_q,
                                 const int32_t* pair_d, const float* idf, const int64_t* list_offsets_host, int n_lists, int Q, int L,
                                 const float* packed, int64_t V, int D, int topk, const float* gate_w, const float* ffw_w, const float* ffw_b,
                                 const float* out_w, const float* out_b, float* out, int* status, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* PACRR the same way (the float form of the table, then capamd_pacrr_forward's MFMA kernel with a table lookup per position as its front
 * end): scores bit-identical to capamd_pacrr_forward's.  Q <= 4, nfilters <= 32, maxgram <= 3, L <= 1024. */
int capamd_pacrr_forward_lists(const int64_t* q_ids, const int64_t* d_ids, const int32_t* q_table, const int32_t* d_table, const int32_t* pair_q,
                               const int32_t* pair_d, const float* idf, const int64_t* list_offsets_host, int n_lists, int Q, int L,
                               const float* packed, int64_t V, int D, int mingram, int maxgram, int nfilters, int kmax, const float* conv_w,
                               const float* conv_b, int use_idf, int combine, int nonlinearity, const float* w1, const float* b1, const float* w2,
                               const float* b2, const float* w3, const float* b3, float* out, int* status, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ---- DRMMTKS_class.forward (capreolus/reranker/DRMMTKS.py:50-64) behind DRMMTKS.test (:105-110) ------------------
 * A sibling of DRMM on the same fused front end: per query term the top-k similarities over all
 * L positions -> Linear(topk, 1) + tanh (ffw_w fp32 [topk], ffw_b [1]) -> IDF gate (gate_w [1]) -> output layer.
 * topk <= 16, topk <= L, Q <= 32.  Only gateType = IDF (the reference's TV branch feeds integer ids to nn.Linear). */
int capamd_drmmtks_forward(const int64_t* q_ids, const int64_t* d_ids, const float* idf, int B, int Q, int L,
                           const float* packed, int64_t V, int D, int topk, const float* gate_w, const float* ffw_w,
                           const float* ffw_b, const float* out_w, const float* out_b, float* out, int* status, void* stream);
/* Training-step half of DRMM-TKS (row N3; reference trainer/pytorch.py:96-99 -> DRMMTKS.score): features[B][Q][topk] = the sorted
 * top-k similarities of every query term (DRMMTKS.py:55-56).  The embedding table is frozen (freezeemb), so no gradient flows
 * through them; the Linear(topk,1)/tanh, the idf gate and the output layer (a few dozen flops per pair) run under autograd. */
int capamd_drmmtks_features(const int64_t* q_ids, const int64_t* d_ids, int B, int Q, int L, const float* packed, int64_t V, int D,
                            int topk, float* features, int* status, void* stream);

/* One DRMM-TKS training step on the device (see capamd_knrm_train_step; reference DRMMTKS.py:50-64 under trainer/pytorch.py:93-108): top-k
 * features of the 2 B documents, Linear(topk, 1) / tanh, softmax idf gate, output layer, the pairwise loss (0 hinge / 1 softmax), backward and
 * torch.optim.Adam's in-place update, in two launches.  ptrs: DEVICE array of 3 x 5 device pointers - ffw.0.weight [topk], ffw.0.bias [1],
 * gates.weight [1], output_layer.weight [1], output_layer.bias [1], then their exp_avg, then their exp_avg_sq.  idf: [B, Q] of the queries.
 * workspace: capamd_drmmtks_train_step_workspace_floats(B, Q, topk) floats.  B <= 1024. */
size_t capamd_drmmtks_train_step_workspace_floats(int B, int Q, int topk);
int capamd_drmmtks_train_step(const int64_t* q_ids, const int64_t* pos_ids, const int64_t* neg_ids, const float* idf, int B, int Q, int L,
                              const float* packed, int64_t V, int D, int topk, float* const* ptrs, int loss_type, float step_size,
                              float one_minus_beta1, float beta2, float eps, float bc2_sqrt, float* loss_out, float* workspace,
                              size_t workspace_floats, int* status, void* stream);

/* ---- PTBERTMaxP_Class.predict_step (capreolus/reranker/ptBERTMaxP.py:67-96) behind PTBERTMaxP.test
 * (ptBERTMaxP.py:134-135), including the transformers.BertForSequenceClassification forward it calls
 * at :82 (embeddings, 12 post-LN encoder layers, pooler, classifier, logit 1).
 *
 * The model is described by plain pointers.  fp32 tensors are read in place from the live
 * nn.Module parameters; the GEMM weights are converted once to bf16 into a caller-owned `blob`
 * (capamd_bert_pack_layer; re-run it after load_weights / an optimizer step), the per-layer
 * biases and LayerNorm vectors are gathered into `layer_f32`.
 * hidden = 64*heads, hidden % 64 == 0, hidden <= 1024, ffn % 64 == 0; S a multiple of 32 up to 256, or 384, or 512. */
typedef struct capamd_bert_model {
  int hidden, layers, heads, ffn, vocab, max_pos, type_vocab;
  int compute_dtype;      /* 16-bit operand/activation type: 0 = bf16 (default), 1 = fp16 (the reference's amp autocast type;
                             ~8x smaller rounding error, same MFMA rate, narrower range) */
  const float* word_emb;  /* [vocab, hidden]      bert.embeddings.word_embeddings.weight */
  const float* pos_emb;   /* [max_pos, hidden]    bert.embeddings.position_embeddings.weight */
  const float* type_emb;  /* [type_vocab, hidden] bert.embeddings.token_type_embeddings.weight */
  const float* emb_ln_g;  /* [hidden]             bert.embeddings.LayerNorm.weight */
  const float* emb_ln_b;  /* [hidden]             bert.embeddings.LayerNorm.bias */
  const float* pooler_w;  /* [hidden, hidden]     bert.pooler.dense.weight */
  const float* pooler_b;  /* [hidden] */
  const float* cls_w;     /* [2, hidden]          classifier.weight */
  const float* cls_b;     /* [2] */
  const void* blob;       /* capamd_bert_blob_bytes(): per layer Wqkv[3H,H] | Wo[H,H] | W1[F,H] | W2[H,F] (+ gamma-scaled Wqkv, W1), 16-bit */
  const float* layer_f32; /* layers * capamd_bert_layer_f32_floats(): bqkv | bo | ln1.g | ln1.b | b1 | b2 | ln2.g | ln2.b | folded-LayerNorm vectors */
  /* RoBERTa bodies (transformers.RobertaForSequenceClassification behind ptBERTMaxP.py:46-48, 57-58): the same encoder with
   *   - position ids counted over the non-pad tokens: pad_id + #(ids[0..i] != pad_id) for a non-pad token, pad_id for a pad
   *     (pos_pad_id >= 0; -1 = BERT: position i),
   *   - its own LayerNorm epsilon (1e-5; 0 = BERT's 1e-12),
   *   - a `dense -> tanh -> out_proj` head on the first token: the pooler / classifier arithmetic under other names
   *     (pooler_w/b = classifier.dense, cls_w/b = classifier.out_proj) and a one-row token-type table. */
  float ln_eps;
  int pos_pad_id;
} capamd_bert_model;

int64_t capamd_bert_blob_bytes(const capamd_bert_model* m);        /* only the int fields are read */
int64_t capamd_bert_layer_f32_floats(const capamd_bert_model* m);  /* floats per layer */
/* tensors_host: HOST array of 18 DEVICE pointers for encoder layer `layer`, in this order:
 * attention.self.query.{weight,bias}, .key.{weight,bias}, .value.{weight,bias}, attention.output.dense.{weight,bias},
 * attention.output.LayerNorm.{weight,bias}, intermediate.dense.{weight,bias}, output.dense.{weight,bias},
 * output.LayerNorm.{weight,bias}, and [16], [17] = {weight, bias} of the LayerNorm whose output is this layer's input
 * (the previous layer's output.LayerNorm; both NULL for layer 0, which reads the normalised embeddings).  The last
 * two are folded into this layer's QKV and attention-output epilogues (LayerNorm fused into the GEMMs: weights
 * pre-scaled by gamma, per-column sums and folded biases stored behind the plain vectors of `layer_f32`). */
int capamd_bert_pack_layer(const capamd_bert_model* m, int layer, const float* const* tensors_host, void* blob,
                           float* layer_f32, void* stream);
/* workspace for scoring `total_passages` = B*P passages in micro-batches of `passages_per_microbatch` */
int64_t capamd_bert_workspace_bytes(const capamd_bert_model* m, int S, int64_t passages_per_microbatch,
                                    int64_t total_passages);
/* ids/mask/seg int64 [B, P, S] (bertpassage.py:313-325); aggregation 0 max, 1 first, 2 sum, 3 avg
 * (ptBERTMaxP.py:85-94; avg divides by the batch-wide passage count as the reference does);
 * out fp32 [B]; passage_logits_out optional fp32 [B*P]; workspace 256-byte aligned. */
int capamd_bert_maxp_forward(const int64_t* ids, const int64_t* mask, const int64_t* seg, int B, int P, int S,
                             const capamd_bert_model* m, int aggregation, int64_t passages_per_microbatch,
                             void* workspace, int64_t workspace_bytes, float* out, float* passage_logits_out,
                             int* status, void* stream);

/* The passage pooling of predict_step alone (capreolus/reranker/ptBERTMaxP.py:75-94) over fp32 passage logits [B*P]:
 * aggregation 0 max, 1 first, 2 sum, 3 avg, with passage_mask = (sum(mask*seg) > 5) from the FULL [B,P,S] mask / seg
 * arrays.  Used when the passages of a call are encoded in length buckets (capreolus_amd.engine.BertEngine,
 * skip_padding): passages are independent and padded positions never reach a real token, so a passage whose tokens end
 * before position 32k can be encoded at S = 32k (any supported length) with bit-identical logits.  count_scratch: 4 bytes. */
int capamd_maxp_pool(const float* passage_logits, const int64_t* mask, const int64_t* seg, int B, int P, int S, int aggregation,
                     float* out, int* count_scratch, void* stream);

/* Encoder building blocks (what BertSelfAttention / nn.Linear + activation compute inside the HF model
 * the reference calls at ptBERTMaxP.py:82).  16-bit (bf16 or fp16) operands, fp32 accumulation.
 * capamd_bert_gemm: out[M,N] = A[M,K] · W[N,K]^T + bias, epilogue 0: bf16 out; 1: erf-GELU, bf16 out;
 * 4: + resid[M,N] (bf16), bf16 out (fp32 sum, one rounding).  M, N, K multiples of 64.
 * Layout bits OR-ed into `epilogue` (M, N multiples of 256, K >= 128; not with epilogue 4): the engine's internal
 * "chunk-major" activation layout of a [R][C] 16-bit tensor - blocks of 32 rows, inside a block the 16-byte chunks
 * of one column position of all 32 rows contiguous:  (r, c) -> (((r/32)*(C/8) + c/8)*32 + r%32)*8 + c%8.
 * Its producers store straight from MFMA registers (no LDS regrouping), its consumers still fetch full 128-byte lines. */
#define CAPAMD_GEMM_A_CHUNK_MAJOR 0x200   /* A is chunk-major */
#define CAPAMD_GEMM_OUT_CHUNK_MAJOR 0x100 /* out is chunk-major */
#define CAPAMD_GEMM_RING_256 0x800         /* with W chunk-major: the ring kernel's 256-row tile (one workgroup per CU) instead of its default 128-row tile (two per CU);
                                            with a chunk-major output and K % 64 == 0 that tile runs on 16x16x32 MFMAs (k accumulated in steps of 32: not the
                                            bits of the other kernels, which accumulate in steps of 16) */
#define CAPAMD_GEMM_RING_MFMA16 0x2000     /* without CAPAMD_GEMM_RING_256: the 128-row tile (two workgroups per CU) on 16x16x32 MFMAs too (chunk-major output, K % 64 == 0;
                                            not for the QKV epilogue) - the bits of the 256-row 16x16x32 tile */
#define CAPAMD_GEMM_RING_MFMA32 0x1000     /* with CAPAMD_GEMM_RING_256: keep the 256-row tile on 32x32x16 MFMAs (the bits of the 128-row tile and the 8-wave kernel) */
#define CAPAMD_GEMM_W_CHUNK_MAJOR 0x400   /* W is chunk-major too (with A chunk-major, M, N % 256 == 0, K % 32 == 0, K >= 256: the 4-wave ring kernel) */
int capamd_bert_gemm(const void* A, const void* W, const float* bias, int M, int N, int K, int epilogue,
                     const void* resid, void* out, int dtype /* 0 bf16, 1 fp16 */, void* stream);
/* The same GEMM with LayerNorm folded in (what capamd_bert_maxp_forward runs on BERT-base shapes; exported for the unit
 * tests).  M, N multiples of 256, K >= 128 and a multiple of 64.  `epilogue`: 0 / 1 as above, or 5, plus the layout bits.
 * Consumer side (ln_mu != NULL): A holds UN-normalised rows P, W = W0 . gamma (column-scaled), ln_cs[n] = sum_k W[n][k],
 *   bias[n] = b[n] + sum_k beta[k] W0[n][k]; the epilogue computes rstd_m (acc - mu_m cs_n) + bias_n == LN(P) W0^T + b.
 *   ln_mu, ln_rstd fp32 [M]; ln_mr fp32 [M][2] the same two interleaved.
 * Producer side (epilogue 5, chunk-major out): out = acc + bias + (R - mu_m) rstd_m gamma_n with R = res_src [M, N] chunk-major,
 *   res_mr [M][2] its (mu, rstd), res_gamma [N]; stat_part fp32 [M][N/64][2] receives (sum, sum of squares) of the rounded
 *   output over each 64-column slice (fixed slots, no atomics). */
int capamd_bert_gemm_ln(const void* A, const void* W, const float* bias, int M, int N, int K, int epilogue, const float* ln_mu,
                        const float* ln_rstd, const float* ln_mr, const float* ln_cs, const void* res_src, const float* res_mr,
                        const float* res_gamma, float* stat_part, void* out, int dtype, void* stream);
/* x bf16 [n_passages*S, hidden] -> fused QKV projection (+bias, Q/8) -> softmax(QK^T + pad mask) V.
 * q, k: bf16 [n_passages*S, hidden]; vt: bf16 [n_passages*heads, 64, S]; ctx: bf16 [n_passages*S, hidden];
 * mask int64 [n_passages, S]. */
int capamd_bert_qkv_attention(const void* x, const void* wqkv, const float* bqkv, const int64_t* mask, int n_passages,
                              int S, int hidden, int heads, void* q, void* k, void* vt, void* ctx, int dtype, void* stream);

/* ---- CEDR-KNRM -----------------------------------------------------------------------
 * Replaces CEDRKNRM_Class.forward, capreolus/reranker/CEDRKNRM.py:151-185 (called from CEDRKNRM.test :216-217), BERT-architecture
 * encoders only.  Two calls:
 *  capamd_cedr_passage_features: runs the encoder (same model / workspace as capamd_bert_maxp_forward; the pooler and classifier
 *   pointers of the model may be NULL) over all B*P passages and, for every hidden state listed in simmat_layers (host array,
 *   0 = embedding output .. layers), leaves passage_kernel_sums[layer][passage][kernel][query row] =
 *   sum over the passage's document tokens of the RBF kernels of the masked cosine similarity matrix (masked_simmats /
 *   _cos_simmat / knrm, CEDRKNRM.py:83-130; query rows = sequence positions 1..maxqlen+1), plus cls_rows[passage][hidden] = the
 *   last hidden state's [CLS] row in fp32 (:160).  query_mask0 [B*P][maxqlen+1] (fp32 0/1): for every passage, the query mask
 *   (attention mask & segment 0 at sequence positions 1..maxqlen+1) of the FIRST passage of its document - the mask the
 *   reference applies to all of a document's passages (:123); handing it in per passage lets a caller regroup passages (e.g. by
 *   length, with P = 1) without losing their document.  maxqlen + 1 <= 32, K <= 11.
 *  capamd_cedr_score: the document level (:117-136, 160-185): sums over a document's P passages, clamp / log / 0.01, sum over
 *   the query rows; cls feature (cls_mode 0 none, 1 avg, 2 max); combine = Linear(n_in, 1) (combine_hidden = 0) or
 *   Linear(n_in, combine_hidden) -> Linear(combine_hidden, 1).  features_out (optional) [B][n_in]. */
int capamd_cedr_passage_features(const int64_t* ids, const int64_t* mask, const int64_t* seg, int B, int P, int S,
                                 const capamd_bert_model* m, int64_t passages_per_microbatch, void* workspace, int64_t workspace_bytes,
                                 int maxqlen, const float* query_mask0, const int* simmat_layers, int n_layers, const float* mu,
                                 const float* sigma, int K, float* passage_kernel_sums, float* cls_rows, int* status, void* stream);
int capamd_cedr_score(const float* passage_kernel_sums, const float* cls_rows, int B, int P, int maxqlen, int n_layers, int K, int hidden,
                      int cls_mode, const float* w1, const float* b1, int combine_hidden, const float* w2, const float* b2, float* out,
                      float* features_out, void* stream);
/* The tap of capamd_cedr_passage_features alone, on one hidden state of the caller's making (exported for the unit tests; the same
 * launch code as inside the encoder).  x, 16-bit (dtype 0 bf16, 1 fp16), 16-byte aligned (CAPAMD_ERR_ALIGN), by `layout`:
 *   0  row-major hidden state [np*S][hidden]                                        (hidden % 64 == 0, 64..1024; mr NULL)
 *   1  chunk-major (capamd_bert_gemm above), already normalised                     (hidden % 256 == 0; mr NULL)
 *   2  chunk-major pre-LayerNorm sums; mr [np*S][2] = (mu, rstd) of every row, gamma / beta [hidden]: the hidden state is
 *      fma((float(x) - mu) * rstd, gamma, beta) rounded to the 16-bit type, formed in registers
 * mask, seg [np][S] are the micro-batch's own rows; query_mask0 [NP][maxqlen+1] and passage_kernel_sums [NP][K][maxqlen+1] are
 * indexed by p0 + p, as in the encoder: rows p0 .. p0+np-1 are written, no other.  CAPAMD_ERR_ARG: S not a supported length,
 * maxqlen + 1 > 32, maxqlen + 2 > S, K outside 1..11, p0 + np > NP, np < 1, a layout's conditions above, more than 160 KiB of LDS. */
int capamd_cedr_pool(const void* x, int layout, const float* mr, const float* gamma, const float* beta, const int64_t* mask,
                     const int64_t* seg, const float* query_mask0, int64_t p0, int64_t np, int64_t NP, int S, int hidden, int maxqlen,
                     const float* mu, const float* sigma, int K, float* passage_kernel_sums, int dtype, void* stream);

/* ---- PARADE (reference capreolus/reranker/ptparade.py, aggregation = "transformer") -----------------------------------------
 * Replaces PTParade_Class.forward (:66-78, called from PTParade.test).  Two calls:
 *  capamd_parade_passage_cls: runs the encoder (same model / workspace / micro-batch arguments as capamd_bert_maxp_forward; the
 *   pooler and classifier pointers may be NULL) over all B*P passages and leaves cls_rows [B*P][hidden] = the [CLS] row of the last
 *   hidden state in fp32 (:74, before any pooler).  The last layer is computed on the [CLS] rows only.
 *  capamd_parade_head: the aggregation head (:53-65, 78) in fp32 throughout:
 *   X0[b] = [initial_cls; cls_rows of document b] + pos_emb   ([P+1, hidden]),
 *   X2 = BertLayer_2(BertLayer_1(X0)) (post-LN BERT layers, no attention mask, 1/sqrt(64) scaling, erf-GELU),
 *   out[b] = linear_w . X2[b][0] + linear_b[0];  aggregated_out (optional) [B][hidden] = X2[b][0].
 *   hidden = 64*heads <= 1024, ffn % 64 == 0, 1 <= P, P + 1 <= 64; tensors 16-byte aligned (CAPAMD_ERR_ALIGN otherwise).
 * The parameters are read in place from the live fp32 tensors; layer1 / layer2 hold the 16 tensors of a BertLayer in the order of
 * capamd_bert_pack_layer's first 16 (query, key, value, attention.output.dense, attention.output.LayerNorm, intermediate.dense,
 * output.dense, output.LayerNorm; weight before bias). */
typedef struct capamd_parade_head_model {
  const float* initial_cls;  /* [hidden]          initial_cls_embedding */
  const float* pos_emb;      /* [P + 1, hidden]   full_position_embeddings */
  const float* layer1[16];   /* transformer_layer_1.* */
  const float* layer2[16];   /* transformer_layer_2.* */
  const float* linear_w;     /* [1, hidden]       linear.weight */
  const float* linear_b;     /* [1]               linear.bias */
  int hidden, heads, ffn;
  float ln_eps;              /* the layers' LayerNorm epsilon (1e-12 for BERT and ELECTRA) */
} capamd_parade_head_model;

/* workspace for capamd_parade_head over B documents of P passages; -1 for an unsupported geometry (only the int fields are read) */
int64_t capamd_parade_workspace_bytes(const capamd_parade_head_model* hm, int B, int P);
int capamd_parade_passage_cls(const int64_t* ids, const int64_t* mask, const int64_t* seg, int B, int P, int S, const capamd_bert_model* m,
                              int64_t passages_per_microbatch, void* workspace, int64_t workspace_bytes, float* cls_rows, int* status,
                              void* stream);
int capamd_parade_head(const float* cls_rows, int B, int P, const capamd_parade_head_model* hm, void* workspace, int64_t workspace_bytes,
                       float* out, float* aggregated_out, void* stream);

/* ---- Birch (reference capreolus/reranker/birch.py, Birch_Class.forward / score_passages :72-127) ----------------------------------
 * (added without a new CAPAMD_VERSION: purely additive, nothing existing changed)
 * The passage scores are capamd_bert_maxp_forward's passage logits (BertForNextSentencePrediction is the pooler and a [2, hidden]
 * classifier under another name; cls_w / cls_b = cls.seq_relationship).  Two calls stand around the encoder:
 *  capamd_birch_plan: ids / mask / seg int64 [B][P][S] -> which passages are encoded and how (:92-109), per document:
 *   valid[p] = #(seg + mask == 2) > 2, and valid[0] when no passage is valid; the valid passages keep their order (rank 0, 1, ...);
 *   sub-batch g = the passages of rank g subbatch .. (g + 1) subbatch - 1; its cut = the largest, over its passages, of the FIRST
 *   position of the maximum of seg + mask (what argmax returns: the first token of segment B where there is one).  truncate 1: the mask
 *   of a passage is cleared behind its sub-batch's cut (the reference slices the sub-batch there; a key behind the cut gets no
 *   weight either way); truncate 0: nothing is cleared and subbatch has no effect.
 *   enc_ids / enc_mask / enc_seg int64 [B P][S]: rows 0 .. n_enc - 1 are written - the valid passages document after document, the
 *   rows of document b at doc_first[b] .. doc_first[b + 1] - 1; doc_first int32 [B + 1] and n_enc int32 [1] on the device.
 *   workspace: capamd_birch_workspace_bytes(B, P) bytes, 256-byte aligned.
 *  capamd_birch_head: enc_logits fp32 [n_logits] (the encoder's logits of the n_logits = n_enc compacted rows) + doc_first -> per
 *   document the P passage scores (its encoded logits, then their minimum for the passages that were not encoded, :121-125), the topk
 *   largest in descending order (a selection: the values' own bits; equal values in any order; NaN ranks above everything and is the
 *   minimum of a document that has one, as torch.topk / torch.min have it), and combine (:41-47, 82):
 *     hidden == 0:  out[b] = sum_i w1[i] top[i]                        w1 = combine.weight [1][topk]; b1, w2, b2 unused
 *     hidden  > 0:  out[b] = b2[0] + sum_j w2[j] relu(b1[j] + sum_i w1[j][i] top[i])     w1 = combine.0.weight [hidden][topk], w2 = combine.2.weight
 *   read in place from the live fp32 tensors; sums in ascending i, the hidden units reduced in a fixed order: a document's score is a
 *   function of its own logits alone.  topk_out (optional) [B][topk]; passage_scores_out (optional) [B][P].  A document whose
 *   doc_first range is empty or leaves [0, n_logits) scores what lies inside it (0 for none); nothing is read outside enc_logits.
 * Limits (CAPAMD_ERR_ARG, nothing is launched; capamd_birch_workspace_bytes returns -1): 1 <= topk <= P <= 64, 0 <= hidden <= 256,
 * 1 <= subbatch, S a length of capamd_bert_maxp_forward (multiples of 32 up to 256, 384, 512), B P < 2^31, truncate 0 or 1. */
int64_t capamd_birch_workspace_bytes(int B, int P);
int capamd_birch_plan(const int64_t* ids, const int64_t* mask, const int64_t* seg, int B, int P, int S, int subbatch, int truncate, void* workspace,
                      int64_t workspace_bytes, int64_t* enc_ids, int64_t* enc_mask, int64_t* enc_seg, int* doc_first, int* n_enc, void* stream);
int capamd_birch_head(const float* enc_logits, int64_t n_logits, const int* doc_first, int B, int P, int topk, int hidden, const float* w1,
                      const float* b1, const float* w2, const float* b2, float* out, float* topk_out, float* passage_scores_out, void* stream);

/* ---- TK (reference capreolus/reranker/TK.py, TK_class.forward :124-143, called from TK.test) ------------------------------------
 * score[b] of query ids q_ids [B, Q] against document ids d_ids [B, L] (int64), fp32 throughout:
 *   x = emb[id] + pe[position]; numlayers post-norm TransformerEncoderLayers (ReLU, LayerNorm eps ln_eps, no dropout), the query and
 *   the document encoded as separate sequences; usemask != 0: a position whose embedding row is all zeros is excluded as query and as
 *   key of the attention of its own sequence (a row that attends to nothing gets a zero attention output);
 *   e = a emb[id] + (1 - a) x_final with a = *mixer (mixer != NULL) or alpha; cosine of every (query, document) position pair, 0 where
 *   either id equals `pad`; the 11 kernels exp(-(c - mu)^2) / (2 sigma^2) (mu = -0.9, -0.7, .., 0.9, 1.0, sigma = 0.1) summed over
 *   all L positions; s_log_k = sum_q log2(.), s_len_k = sum_q (.) / L; score = comb_w . [s_log_w . s_log_k, s_len_w . s_len_k].
 *   features_out (optional) [B][22] = s_log_k, s_len_k.
 * Weights in the padded layout (built once per set of weights by the caller; every pad element 0, tensors 16-byte aligned):
 *   Dp = roundup(dim, 64), hd = dim / heads, hs = roundup(hd, 16), Hs = roundup(heads * hs, 64), Fp = roundup(ffdim, 64);
 *   wqkv [3 Hs][Dp]: row p Hs + h hs + j (p = q, k, v; j < hd) = in_proj_weight row p dim + h hd + j;  bqkv [3 Hs] likewise;
 *   wo [Dp][Hs]: column h hs + j = out_proj.weight column h hd + j;  bo, ln1_*, ln2_*, b2 [Dp];  w1 [Fp][Dp], b1 [Fp];  w2 [Dp][Fp].
 * emb [vocab][dim] and pe [max_len][dim] (position_encoder.pe) are read in place; ids outside [0, vocab) are scored as a zero row and
 * set CAPAMD_STATUS_DOC_ID_RANGE / _QUERY_ID_RANGE (nn.Embedding raises).  Limits: dim <= 512, dim % heads == 0, hd <= 64,
 * ffdim <= 512, numlayers >= 1, 1 <= Q <= 32, 1 <= L <= max_len.  Documents run in micro-batches of docs_per_microbatch; the
 * workspace (256-byte aligned) is capamd_tk_workspace_bytes(m, docs_per_microbatch, Q, L) bytes (-1: unsupported geometry).  Each
 * document's score is independent of the micro-batch size and of the other documents of the call, bit for bit. */
typedef struct capamd_tk_layer {
  const float *wqkv, *bqkv, *wo, *bo, *ln1_g, *ln1_b, *w1, *b1, *w2, *b2, *ln2_g, *ln2_b;
} capamd_tk_layer;
typedef struct capamd_tk_model {
  const float* emb;                      /* [vocab][dim]    embedding.weight */
  const float* pe;                       /* [max_len][dim]  position_encoder.pe */
  const capamd_tk_layer* layers_host;    /* [numlayers], a HOST array of device pointers */
  const float* mixer;                    /* [1] the mixer parameter (usemixer), or NULL: alpha */
  const float *s_log_w, *s_len_w, *comb_w;   /* [11], [11], [2] */
  int64_t vocab, pad;
  int dim, heads, ffdim, numlayers, max_len, usemask;
  float alpha, ln_eps;
} capamd_tk_model;

int64_t capamd_tk_workspace_bytes(const capamd_tk_model* m, int docs_per_microbatch, int Q, int L);
int capamd_tk_forward(const int64_t* q_ids, const int64_t* d_ids, int B, int Q, int L, const capamd_tk_model* m, int docs_per_microbatch,
                      void* workspace, int64_t workspace_bytes, float* out, float* features_out, int* status, void* stream);

/* ---- HINT (reference capreolus/reranker/HINT.py, HiNT_main.test_forward -> HiNT.forward, called from HINT.test) -------------------
 * score[b] of query ids q_ids [B, Q] against document ids d_ids [B, L] (int64), fp32 throughout.  P = L / 100 windows of 100 terms
 * (the reference's hard-coded width); the terms behind P x 100 are not read.  Per window and query term i, document term j:
 *   cos_ij = (q_i / (|q_i| + 1e-7)) . (d_j / (|d_j| + 1e-7));  xor_ij = 1 where the ids are equal (pad against pad included);
 *   channels [Ws q_i + b, Ws d_j + b, M_ij], all three zeroed where BOTH ids are 0;
 *   the spatial GRU (GRUCell2d, hidden 2) over the Q x 100 cells, query rows outside, its last cell's state: gru1 on the xor and the
 *   cos tensor, gru3 on both with both axes reversed -> 8 values per window [H_xor, H_cos, H_xor_inv, H_cos_inv];
 *   a bidirectional LSTM (hidden 6) over the P windows from zero state, forward + backward; tanh(Wv .); the 2P rows [vt; lstm]
 *   top-kmax sorted per hidden unit, flattened unit * kmax + rank; fc.
 * The parameters are read in place from the live fp32 tensors in nn.Linear / nn.LSTM layout: ws_w [dim], ws_b [1]; per GRU cell
 * wrz_w [14][9], wrz_b [14], w_w [2][3], w_b [2], u_w [2][6], u_b [2]; lstm_w_ih [24][8], lstm_w_hh [24][6], lstm_b_ih / _b_hh [24]
 * (gates i, f, g, o) and the *_r set of the reverse direction; wv_w [6][8], wv_b [6]; fc_w [6 kmax], fc_b [1].
 * emb [vocab][dim] is read in place; ids outside [0, vocab) are scored as a zero row and set CAPAMD_STATUS_DOC_ID_RANGE /
 * _QUERY_ID_RANGE (nn.Embedding raises).  Limits: 1 <= dim <= 512, 1 <= Q <= 32, 100 <= L, P <= 64, 1 <= kmax <= min(2 P, 32).
 * Documents run in micro-batches of docs_per_microbatch; the workspace (256-byte aligned) is
 * capamd_hint_workspace_bytes(m, docs_per_microbatch, Q, L) bytes (-1: unsupported geometry).  evidence_out (optional) [B][P][8]: the
 * LSTM's input.  Each document's score is independent of the micro-batch size and of the other documents of the call, bit for bit. */
typedef struct capamd_hint_gru {
  const float *wrz_w, *wrz_b, *w_w, *w_b, *u_w, *u_b;
} capamd_hint_gru;
typedef struct capamd_hint_model {
  const float* emb;                      /* [vocab][dim]    HiNT1.embedding.weight */
  const float *ws_w, *ws_b;              /* HiNT1.Ws */
  capamd_hint_gru gru1, gru3;            /* HiNT1.GRU2d1.gru_cell, HiNT1.GRU2d3.gru_cell */
  const float *lstm_w_ih, *lstm_w_hh, *lstm_b_ih, *lstm_b_hh;           /* HiNT1.lstm.*_l0 */
  const float *lstm_w_ih_r, *lstm_w_hh_r, *lstm_b_ih_r, *lstm_b_hh_r;   /* HiNT1.lstm.*_l0_reverse */
  const float *wv_w, *wv_b, *fc_w, *fc_b;
  int64_t vocab;
  int dim, kmax;
} capamd_hint_model;

int64_t capamd_hint_workspace_bytes(const capamd_hint_model* m, int docs_per_microbatch, int Q, int L);
int capamd_hint_forward(const int64_t* q_ids, const int64_t* d_ids, int B, int Q, int L, const capamd_hint_model* m, int docs_per_microbatch,
                        void* workspace, int64_t workspace_bytes, float* out, float* evidence_out, int* status, void* stream);

/* ---- POSITDRMM (reference capreolus/reranker/POSITDRMM.py, POSITDRMM_class.test_forward -> POSITDRMM_basic.forward) ---------------
 * score[b] of query ids q_ids [B, Q] (idf q_idf [B, Q] fp32) against document ids d_ids [B, L] (int64), fp32 throughout:
 *   M_cos_ij = (q_i / (|q_i| + 1e-7)) . (d_j / (|d_j| + 1e-7));  xor_ij = 1 where the ids are equal and q_i != pad;
 *   the 2-layer bidirectional LSTM (hidden = dim, gates i, f, g, o, no dropout) from zero state over the Q query positions and over
 *   ALL L document positions, pads included; context rows [fwd + x, bwd + x]; M_ctx_ij = their cosine, no epsilon;
 *   per query term the max and the mean of the 5 largest over j of M_cos, M_ctx, xor -> 6 features; LeakyReLU(0.01)(Q1 .);
 *   ans = sum_i softmax(q_idf)_i . ;  score = Wg [ans, extras(4)].
 * extras [B][4], or NULL: then [s0, s1, s2, bm25[b]] with the reference's get_exact_match_stats computed here from the ids (the query
 * as it is, the document without its pads; len = its non-pad terms): s0 = matches / len, s1 = sum_i (matches of q_i) idf_i / len
 * (summed in query order in fp32), s2 = matches of query bigrams among the cleaned document's bigrams / (len - 1).  They are always
 * computed; len < 2 sets CAPAMD_STATUS_SHORT_DOC (the three are then 0).
 * Weights in the padded layout (built once per set of weights by the caller; every pad element 0, 16-byte aligned), Dp =
 * roundup(dim, 64), both directions back to back (forward, reverse), gate rows reordered: packed row ub 64 + g 16 + j = row g dim + u
 * of the nn.LSTM tensor (g = 0..3: i, f, g, o; u = ub 16 + j < dim);
 *   w_ih[0] [2][4 Dp][Dp]; w_ih[1] [2][4 Dp][2 Dp] with the input columns dim .. 2 dim - 1 at Dp ..; bias[l] [2][4 Dp] = bias_ih + bias_hh;
 *   w_hh[l] [2][4 Dp x Dp], its packed rows stored fragment-major for the recurrence's MFMA loads: [ub][k / 16][g][lane 0..63][4] holds
 *   packed row ub 64 + g 16 + (lane & 15), columns 16 (k / 16) + 4 (lane >> 4) .. + 3.
 * emb [vocab][dim], q1_w [6], q1_b [1], wg_w [5], wg_b [1] are read in place; ids outside [0, vocab) are scored as a zero row and set
 * CAPAMD_STATUS_DOC_ID_RANGE / _QUERY_ID_RANGE.  Limits: 1 <= dim <= 320, 1 <= Q <= 16, 5 <= L <= 8192, docs_per_microbatch <= 2^20.
 * Pairs run in micro-batches of docs_per_microbatch; the workspace (256-byte aligned) is capamd_posit_workspace_bytes(m,
 * docs_per_microbatch, Q, L) bytes (-1: unsupported geometry; about 16 Dp (L + Q) + 8 Q L bytes per pair plus 512 MiB of input
 * projections).  Optional outputs: features_out [B][Q][6] (the input of Q1), stats_out [B][3], qctx_out [B][Q][2 dim], dctx_out
 * [B][L][2 dim] (the context rows).  Each pair's results are independent of the micro-batch size and of the other pairs of the call,
 * bit for bit. */
typedef struct capamd_posit_model {
  const float* emb;                      /* [vocab][dim]    posit1.embedding.weight */
  const float* w_ih[2];                  /* per layer, packed (above) */
  const float* w_hh[2];
  const float* bias[2];
  const float *q1_w, *q1_b, *wg_w, *wg_b;   /* posit1.Q1, posit1.Wg */
  int64_t vocab, pad;
  int dim;
} capamd_posit_model;

int64_t capamd_posit_workspace_bytes(const capamd_posit_model* m, int docs_per_microbatch, int Q, int L);
int capamd_posit_forward(const int64_t* q_ids, const float* q_idf, const int64_t* d_ids, const float* extras, const float* bm25, int B, int Q, int L,
                         const capamd_posit_model* m, int docs_per_microbatch, void* workspace, int64_t workspace_bytes, float* out,
                         float* features_out, float* stats_out, float* qctx_out, float* dctx_out, int* status, void* stream);

/* ---- DeepTileBar (reference capreolus/extractor/deeptileextractor.py, create_visualization_matrix -> color_grid, and
 * capreolus/reranker/DeepTileBar.py, DeepTileBar_class.test_forward) -----------------------------------------------------------------
 * Text tiling itself (nltk.TextTilingTokenizer) stays with the caller: these entries take its segment boundaries.
 *
 * capamd_deeptile_color: term ids + segment boundaries -> tiles_out [B][Q][P][C] fp32, the reference's color_grid, quirks included.
 *   q_ids int64 [B][Q] (pad = 0), d_ids int64 [B][L], seg_start int32 [B][P + 1] (segment p of document b is
 *   d_ids[b][seg_start[b][p] .. seg_start[b][p + 1]); the offsets need not cover the row: tokens outside [start[0], start[P]) are
 *   ignored), idf fp32 [B][Q], emb fp32 [V][D] read in place, C = 3 or 2 (the extractor's `tfchannel` false).  Per (query term q, segment):
 *     q == 0 (a pad query term) or an empty segment (start[p] == start[p + 1]: how the host encodes the literal "<pad>" segment that
 *     padlist appends): zeros;  otherwise tf = the segment's tokens whose id equals q, channels [tf, idf if tf else 0, sim] (C = 3) or
 *     [idf if tf else 0, sim] (C = 2), sim = max over the segment's tokens of exp(-|emb[t] - emb[q]|^2 / 2), the squared distance summed
 *     from the differences (not |x|^2 + |z|^2 - 2 x.z), accurate expf;
 *     a token with a NEGATIVE id (the literal "<pad>" token) contributes exactly 0 and is never counted in tf; a token with id 0 (every
 *     word stoi does not know: stoi.get(tok, pad)) is looked up like any other and contributes exp(-|emb[q]|^2 / 2), not 0.
 *   Ids >= V count as the zero row and set CAPAMD_STATUS_DOC_ID_RANGE / _QUERY_ID_RANGE (a negative query id likewise).  Offsets that
 *   decrease or leave [0, L] are clamped to min(L, max(0, start[0..p])) and set CAPAMD_STATUS_SEGMENT_RANGE.
 *   Limits: 1 <= Q <= 32, 1 <= P <= 64, 1 <= D <= 512, L >= 1 (CAPAMD_ERR_ARG beyond them).  No workspace.
 *
 * capamd_deeptile_forward: tiles [B][Q][P][C] -> out [B], one launch; evidence_out (optional) [B][10][hidden]: the last hidden state of
 * each LSTM in order 1 .. 10, the input of W1.  Per document, the tile seen as [C][Q][P]: conv_w (w = 1 .. 10; kernel (Q, w), 3
 * filters, bias, no activation) gives a sequence of T_w = P - w + 1 steps of 3 values; lstm_w (gates i, f, g, o, both biases, zero
 * state) runs over it and only its last h is kept; the ten h concatenated; relu(W1 .), relu(W2 .), W3.
 * The parameters come as ONE fp32 buffer `packed` of capamd_deeptile_packed_floats(m) floats (-1: a configuration that is refused),
 * laid out by the caller once per parameter version: per width w = 1 .. 10 [conv_w.weight [3][C][Q][w] | conv_w.bias [3] |
 * lstm_w.weight_ih_l0 [4 hidden][3] | weight_hh_l0 [4 hidden][hidden] | bias_ih_l0 [4 hidden] | bias_hh_l0 [4 hidden]], then
 * W1.weight [lin1][10 hidden] | W1.bias | W2.weight [lin2][lin1] | W2.bias | W3.weight [lin2] | W3.bias [1].
 * Limits (CAPAMD_ERR_ARG, nothing is launched): filters == 3 (the reference hard-codes nn.LSTM(input_size=3)), 10 <= P <= 64 (conv10
 * needs ten columns), Q == maxqlen, 1 <= maxqlen <= 32, C == channels in {2, 3}, 1 <= hidden <= 16, 1 <= lin1, lin2 <= 128,
 * packed_floats == capamd_deeptile_packed_floats(m).  No workspace: a document's tile is about 1 KB.  Each document's score is
 * independent of the other documents of the call, bit for bit. */
typedef struct capamd_deeptile_model {
  const float* packed;                   /* the layout above */
  int64_t packed_floats;
  int maxqlen, channels, filters, hidden, lin1, lin2;
} capamd_deeptile_model;

int capamd_deeptile_color(const int64_t* q_ids, const int64_t* d_ids, const int* seg_start, const float* idf, int B, int Q, int L, int P,
                          const float* emb, int64_t V, int D, int C, float* tiles_out, int* status, void* stream);
int64_t capamd_deeptile_packed_floats(const capamd_deeptile_model* m);
int capamd_deeptile_forward(const float* tiles, int B, int Q, int P, int C, const capamd_deeptile_model* m, float* out, float* evidence_out,
                            void* stream);

/* ---- DSSM and CDSSM (reference capreolus/reranker/DSSM.py, DSSM_class.forward, and CDSSM.py, CDSSM_class.forward) -------------------
 * Both models are score = sigmoid(cos(tower(query), tower(document))): a tower runs once per distinct row, pairs are scored from the
 * tower outputs.  `side` (0: query rows, 1: document rows) only chooses the status bit of an id outside its table (_QUERY_ID_RANGE /
 * _DOC_ID_RANGE).  fp32 throughout, no workspace.  A row's tower output does not depend on N or on the other rows of the call, bit
 * for bit.
 *
 * capamd_cdssm_tower: ids int64 [N][T] -> rep [N][R] fp32, R = windowsize dim - nkernel + 1, not normalised.  x = emb[ids] (row 0 is read
 *   as the table has it: nothing masks pads), windowsize - T % windowsize zero rows appended (never none: a T that is a multiple gets a
 *   whole window of zeros), the rows cut into K = T / windowsize + 1 windows of windowsize dim floats each, and
 *     rep[t] = max over windows i and filters f of relu(b_f + sum_j w[f][j] x_i[t + j]),  j = 0 .. nkernel - 1,
 *   the taps running across word boundaries inside a window, summed as one fmaf chain from the bias in the order of j.
 *   emb [vocab][dim] is read in place (16-byte aligned), conv_w [nfilter][nkernel] (Conv1d(1, nfilter, nkernel).weight), conv_b [nfilter].
 *   An id outside [0, vocab) counts as a zero row and sets the side's bit.
 *   Limits (CAPAMD_ERR_ARG, nothing is launched): 1 <= dim <= 512, 1 <= windowsize <= 8, windowsize dim <= 4096,
 *   1 <= nkernel <= min(16, windowsize dim), 1 <= nfilter <= 16, T >= 1, 0 <= N < 2^31, side 0 or 1.
 *
 * capamd_dssm_tower: bags of words in CSR form - indptr int64 [N + 1], idx int32 [nnz], val fp32 [nnz]; bag n is the entries
 *   indptr[n] .. indptr[n + 1] - 1 - -> rep [N][width[layers - 1]] fp32, the output of the last ReLU, not normalised:
 *     h_1 = relu(b1 + sum_k val_k W1^T[idx_k]),  h_l = relu(W_l h_(l-1) + b_l).
 *   w1t [nvocab][h1p] is ffw.linear0.weight transposed, its rows padded with zeros to h1p = width[0] rounded up to 64 floats (16-byte
 *   aligned; built once per set of weights by the caller); b1 [width[0]]; w[l - 1] [width[l]][width[l - 1]] and b[l - 1] [width[l]] are
 *   ffw.linear<l> as nn.Linear has them, l = 1 .. layers - 1.  The first layer's sum runs in an order that is a function of the bag alone
 *   (entry k on wave k % 4 in the order of k; the four partial sums added in wave order onto the bias): no float atomics.  An empty
 *   bag is legal (h_1 = relu(b1)).  An idx outside [0, nvocab) is skipped and sets the side's bit; an indptr pair that decreases or
 *   leaves [0, nnz] is clamped (lo into [0, nnz], hi into [lo, nnz]) and sets CAPAMD_STATUS_BAG_RANGE.
 *   Limits (CAPAMD_ERR_ARG): 1 <= layers <= 4, 1 <= width[l] <= 512, 1 <= nvocab < 2^31, 0 <= N < 2^31, side 0 or 1.
 *
 * capamd_cos_sigmoid_pairs: out[i] = sigmoid(dot(q / (|q| + 1e-7), d / (|d| + 1e-7))) of q = qrep[pair_q[i]] ([Nq][R]) and
 *   d = drep[pair_d[i]] ([Nd][R]), each side normalised on its own; pair_q / pair_d int32 [n_pairs], or NULL: then row i (n_pairs <= the
 *   table's rows).  A pair's bits depend on its two rows alone: one query against N documents through the index arrays gives what the
 *   query row repeated N times gives.  An index outside its table counts as a zero row and sets _QUERY_ID_RANGE / _DOC_ID_RANGE.  Two
 *   all-zero rows score exactly 0.5. */
typedef struct capamd_dssm_model {
  const float* w1t;                      /* [nvocab][h1p]   ffw.linear0.weight, transposed and padded (above) */
  const float* b1;                       /* [width[0]]      ffw.linear0.bias */
  const float* w[3];                     /* ffw.linear1 .. linear3 .weight, as nn.Linear has them */
  const float* b[3];
  int64_t nvocab;
  int layers;
  int width[4];
} capamd_dssm_model;

int capamd_cdssm_tower(const int64_t* ids, int64_t N, int T, const float* emb, int64_t vocab, int dim, int windowsize, const float* conv_w,
                       const float* conv_b, int nkernel, int nfilter, int side, float* rep, int* status, void* stream);
int capamd_dssm_tower(const int64_t* indptr, const int* idx, const float* val, int64_t N, int64_t nnz, const capamd_dssm_model* m, int side, float* rep,
                      int* status, void* stream);
int capamd_cos_sigmoid_pairs(const float* qrep, const float* drep, const int* pair_q, const int* pair_d, int64_t Nq, int64_t Nd, int64_t n_pairs, int R,
                             float* out, int* status, void* stream);

/* ---- DUET (reference capreolus/reranker/DUET.py, DUET_class.forward) -------------------------------------------------------------------
 * (added without a new CAPAMD_VERSION: purely additive, nothing existing changed)
 * score = lm + dm per document, fp32 throughout; Q = 4 query terms, H = nfilters, M = lmhidden, act = relu (activation 0) or tanh (1).
 *   local model        lm_x[h][q] = act(lm_b[h] + sum_d W[h][d] (q_ids[q] == d_ids[d]) idf[q])      (idf only with idfweight, else 1)
 *                      lm = lm_w3 . act(lm_w0 flat(lm_x) + lm_b0) + lm_b3,  flat index h Q + q.
 *                      Ids are compared as they are, without any mask: a pad in the query matches every pad in the document, and an id
 *                      outside the table still matches an equal id.  The matching columns are added in ascending d.
 *   distributed model  query:    qv = qf_w max_w act(q_b + conv_(3, dim)(emb[q_ids])[w]) + qf_b over the two windows w of three rows;
 *                      document: c[h][t] = act(d_b1[h] + conv_(3, dim)(emb[d_ids])[h][t]),   t < L - 2
 *                                p[h][t] = max(c[h][t .. t + 99]),                          t < L - 101 (exact)
 *                                e[g][t] = act(d_b2[g] + sum_h d_w2[g][h] p[h][t])
 *                                f[g]    = act(f1_b + sum_t f1_w[t] (qv[g] e[g][t])),        dm = f2_b + sum_g f2_w[g] f[g].
 *                      The table is read as it is (row 0 is not forced to zero); an id outside [0, vocab) counts as a zero row in the
 *                      distributed model and sets CAPAMD_STATUS_QUERY_ID_RANGE / _DOC_ID_RANGE; nothing is read outside the table.
 * Every sum runs in an order that is a function of the document alone (no float atomics): a document's score does not depend on B, on its
 * neighbours or on docs_per_microbatch, bit for bit.
 * Two of the weights are re-laid out by the caller, once per set of weights: lm_wt [maxdoclen][H] is lm.conv.0.weight [H][1][1][maxdoclen]
 * transposed (a position is one contiguous read of H floats); d_w1t [dim rounded up to 32][3 H rounded up to 16] holds
 * dm.d_conv1.0.weight [H][1][3][dim] as d_w1t[k][j H + h] = w[h][j][k], the padding zeros, 16-byte aligned.  Everything else is read in
 * place as nn.Linear / nn.Conv2d have it; emb [vocab][dim] 16-byte aligned.
 * out fp32 [B]; parts_out (optional) fp32 [B][2] = (lm, dm); evidence_out (optional) fp32 [B][H][1 + (L - 101)]: per filter the query
 * vector's entry qv[h], then the pooled row p[h][:].  idf fp32 [B][4] (may be NULL without idfweight).
 * Limits (CAPAMD_ERR_ARG, nothing is launched; capamd_duet_workspace_bytes returns -1): Q == 4, 2 <= nfilters <= 32, 1 <= lmhidden <= 256,
 * 1 <= dim <= 512, 103 <= L <= 8192, nhidden == L - 101, maxdoclen == L - outside the first four the reference itself does not run.
 * workspace: capamd_duet_workspace_bytes(m, docs_per_microbatch, Q, L) bytes, 256-byte aligned: the per-token projections of a micro-batch
 * (L x (3 H rounded up to 16) floats per document). */
typedef struct capamd_duet_model {
  const float* emb;                      /* [vocab][dim]        dm.embedding.weight */
  const float* lm_wt;                    /* [maxdoclen][H]      lm.conv.0.weight, transposed (above) */
  const float* lm_b;                     /* [H]                 lm.conv.0.bias */
  const float *lm_w0, *lm_b0;            /* [M][4 H], [M]       lm.ffw.0 */
  const float *lm_w3, *lm_b3;            /* [M], [1]            lm.ffw.3 */
  const float *q_w, *q_b;                /* [H][3][dim], [H]    dm.q_conv.0 */
  const float *qf_w, *qf_b;              /* [H][H], [H]         dm.q_ffw.0 */
  const float* d_w1t;                    /* dm.d_conv1.0.weight, transposed and padded (above) */
  const float* d_b1;                     /* [H]                 dm.d_conv1.0.bias */
  const float *d_w2, *d_b2;              /* [H][H], [H]         dm.d_conv2.0 */
  const float *f1_w, *f1_b;              /* [nhidden], [1]      dm.ffw_1.0 */
  const float *f2_w, *f2_b;              /* [H], [1]            dm.ffw_2.1 */
  int64_t vocab;
  int dim, nfilters, lmhidden, maxdoclen, nhidden;
  int activation;                        /* 0 relu, 1 tanh */
  int idfweight;
} capamd_duet_model;

int64_t capamd_duet_workspace_bytes(const capamd_duet_model* m, int docs_per_microbatch, int Q, int L);   /* -1: refused geometry */
int capamd_duet_forward(const int64_t* q_ids, const int64_t* d_ids, const float* idf, int B, int Q, int L, const capamd_duet_model* m,
                        int docs_per_microbatch, void* workspace, int64_t workspace_bytes, float* out, float* parts_out, float* evidence_out,
                        int* status, void* stream);

/* ---- ConvKNRM ------------------------------------------------------------------------
 * Replaces ConvKNRM_class.forward, capreolus/reranker/ConvKNRM.py:42-77 (called from ConvKNRM.test :112-116).
 * The Conv1d layers (ConvKNRM.py:24-32) over the frozen embedding table (:17) are folded, once per model, into a table of
 * per-token projections: tables[t][part][f], maxngram*(maxngram+1)/2 parts per token in the order
 *     tap 0 of g = 1..G (bias added) | tap 1 of g = 2..G | tap 2 of g = 3,
 * so that rep_g[j] = part(g,0)[tok j] + part(g,1)[tok j+1] + part(g,2)[tok j+2] (terms beyond the sequence end dropped).
 * conv_w: Conv1d weights of g = 1..maxngram back to back, each [filters][D][g]; conv_b [maxngram][filters].
 * Limits: maxngram <= 3; filters a multiple of 16, 16..128; Q <= 8; K <= 11 kernels; H (hidden width of the two-layer
 * combine, 0 = single Linear) <= 64; L <= 4096.  Ids must lie in [0, V): others set the status bits (nn.Embedding raises).
 * w1 [K*views] (H = 0) or [H][K*views]; feature index = kernel * views + view, view = query_g * G + doc_g (crossmatch) or g. */
int64_t capamd_convknrm_table_bytes(int64_t V, int maxngram, int filters);   /* -1: unsupported geometry */
int capamd_convknrm_pack_tables(const float* emb, int64_t V, int D, int64_t ld, const float* conv_w, const float* conv_b,
                                int maxngram, int filters, float* tables, void* stream);
int capamd_convknrm_forward(const int64_t* q_ids, const int64_t* d_ids, int B, int Q, int L, const float* tables, int64_t V,
                            int maxngram, int filters, int crossmatch, const float* mu, const float* sigma, int K, const float* w1,
                            const float* b1, int H, const float* w2, const float* b2, int score_tanh, float* out, int* status,
                            void* stream);

/* ConvKNRM over whole candidate lists (what PytorchTrainer.predict scores: capreolus/trainer/pytorch.py:310-353 over PredSampler's per-query
 * lists, sampler/__init__.py:222-233): pairs laid out list after list, list l = pairs list_offsets_host[l] .. list_offsets_host[l + 1] (a
 * HOST array of n_lists + 1 entries), every list scored against its FIRST pair's query row (a pair with another row sets
 * CAPAMD_STATUS_LIST_QUERY).  The unigram document view (ConvKNRM.py:46-49 with kernel size 1: a per-token projection) is computed once per
 * DISTINCT token of a list - normalised, multiplied with the list's maxngram x Q query vectors by the same matrix instructions as the
 * per-pair kernel - and looked up per position; the n-gram views of sizes 2 .. maxngram stay per position.  Scores equal
 * capamd_convknrm_forward's bit for bit.  workspace: capamd_convknrm_lists_workspace_bytes(n_lists, V, Q, maxngram, filters) caller-owned
 * bytes (16-byte aligned; per list in flight a flag byte and maxngram x Q floats - rounded up to four - per vocabulary id: 19.6 MB at V =
 * 400,001, Q = 4, maxngram = 3; fewer lists are kept in flight when the buffer is smaller). */
size_t capamd_convknrm_lists_workspace_bytes(int n_lists, int64_t V, int Q, int maxngram, int filters);
int capamd_convknrm_forward_lists(const int64_t* q_ids, const int64_t* d_ids, const int64_t* list_offsets_host, int n_lists, int Q, int L,
                                  const float* tables, int64_t V, int maxngram, int filters, int crossmatch, const float* mu, const float* sigma,
                                  int K, const float* w1, const float* b1, int H, const float* w2, const float* b2, int score_tanh, float* out,
                                  int* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---- PACRR ---------------------------------------------------------------------------
 * Replaces PACRR_class.forward + PACRRConvMax2dModule.forward, capreolus/reranker/PACRR.py:42-78 (called from PACRR.test
 * :114-118): similarity matrix as in KNRM -> per n-gram size Conv2d(1 -> nfilters, ng x ng) on the zero-padded matrix,
 * ReLU, max over filters, kmax largest values over ALL document positions -> optional idf channel (softmax over the
 * query's raw idf values) -> three linear layers with `nonlinearity` (0 none, 1 relu, 2 tanh) in between.
 * conv_w: Conv2d weights of the n-gram modules (mingram..maxgram) back to back, each [nfilters][ng][ng]; conv_b
 * [n_ngrams][nfilters]; w1 [combine][Q * (n_ngrams * kmax + use_idf)], w2 [combine][combine], w3 [combine].
 * Limits: Q <= 8, L <= 1024, maxgram <= 3, kmax <= 4, nfilters <= 256, combine <= 128 (CAPAMD_ERR_ARG beyond them).  Q <= 5
 * with nfilters <= 32 (the reference defaults) runs the convolutions on the matrix pipe (f16 hi/lo split, fp32 accumulate,
 * ~1e-6 of the fp32 form); other geometries an fp32 VALU kernel.  Status bits as for capamd_knrm_forward. */
int capamd_pacrr_forward(const int64_t* q_ids, const int64_t* d_ids, const float* idf, int B, int Q, int L, const float* packed,
                         int64_t V, int D, int mingram, int maxgram, int nfilters, int kmax, const float* conv_w,
                         const float* conv_b, int use_idf, int combine, int nonlinearity, const float* w1, const float* b1,
                         const float* w2, const float* b2, const float* w3, const float* b3, float* out, int* status,
                         void* stream);

/* One PACRR training step on the device (reference PACRR.py:42-78 under trainer/pytorch.py:93-108, the loss
 * reranker/common.py:96-103, torch.optim.Adam): similarity matrices -> n-gram Conv2d / ReLU / max over filters / k-max with the winners'
 * coordinates (capamd_pacrr_convmax_forward) -> ONE workgroup: features + idf softmax, linear1 / linear2 / linear3 with `nonlinearity`
 * (0 none, 1 relu, 2 tanh), the pairwise loss (0 hinge / 1 softmax), the backward through the layers, their gradients summed in document
 * order, Adam on them -> convolution gradients (capamd_pacrr_convmax_backward) -> Adam on the convolutions.  Six launches, no autograd.
 * q_ids int64 [2 B, Q] (the batch's queries twice), d_ids int64 [2 B, L] (positive documents, then negative), idf fp32 [2 B, Q] (use_idf);
 * ptrs: HOST array of 3 P device pointers, P = 2 n_ngrams + 6 - ngrams.{i}.conv.weight / .bias (mingram..maxgram), linear1.weight / .bias,
 * linear2.weight / .bias, linear3.weight / .bias, then their exp_avg, then their exp_avg_sq (null moments: not trained).
 * Limits: those of capamd_pacrr_convmax_*, combine <= 128, and the batch's activations must fit one workgroup's LDS:
 * H X + H^2 + H + 2 B X + 8 B H + 5 B <= 36,864 floats (H = combine, X = Q (n_ngrams kmax + use_idf)); CAPAMD_ERR_ARG beyond.
 * workspace: capamd_pacrr_train_step_workspace_floats(...) floats, 16-byte aligned. */
size_t capamd_pacrr_train_step_workspace_floats(int B, int Q, int L, int mingram, int maxgram, int nfilters, int kmax);
int capamd_pacrr_train_step(const int64_t* q_ids, const int64_t* d_ids, const float* idf, int B, int Q, int L, const float* packed, int64_t V, int D,
                            int mingram, int maxgram, int nfilters, int kmax, int use_idf, int combine, int nonlinearity, float* const* ptrs,
                            int loss_type, float step_size, float one_minus_beta1, float beta2, float eps, float bc2_sqrt, float* loss_out,
                            float* workspace, size_t workspace_floats, int* status, void* stream);

/* ---- ConvKNRM's trainable n-gram convolutions, forward and backward (ConvKNRM's training step) --------------
 * Replaces, for training, the convolution stack of ConvKNRM_class.forward, capreolus/reranker/ConvKNRM.py:42-51 - embeddings(ids) ->
 * permute -> ConstantPad1d((0, g - 1), 0) -> Conv1d(D -> F, kernel g) -> permute, for g = 1..G, on the query and on the document -
 * and its gradient under the reference trainer's loss.backward() (trainer/pytorch.py:96-107): no [B, D, L] embedding tensor, no padded
 * copies, no library convolution - the kernels gather the table's rows and run the g taps as fp32 matrix products on
 * v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate).  The table is frozen (ConvKNRM.py:17): gradients go to the weights and biases only.
 * q_ids int64 [N, Q], d_ids int64 [N, L] (pad = 0; ids outside [0, V) set CAPAMD_STATUS_DOC_ID_RANGE and count as zero rows);
 * emb fp32 [V, D] row-major (nn.Embedding.weight), 16-byte aligned, D % 4 == 0, D <= 316; conv_w / conv_b: HOST arrays of G device
 * pointers, Conv1d weight [F][D][g] and bias [F] of n-gram size g = index + 1; G <= 4; F % 4 == 0, F <= 256.
 * forward:  qrep fp32 [N, G, Q, F], drep fp32 [N, G, L, F].  A 128-position tile without a single real token is written as ZEROS (the
 *           reference's value there is the bias plus the pad row's projection): capamd_kernel_pool_* masks those positions.
 * backward: dqrep / ddrep (16-byte aligned) -> dconv_w / dconv_b (HOST arrays of device pointers, the weights' layouts), overwritten.
 *           Rows of ddrep at pad positions are taken to be zero (what capamd_kernel_pool_backward writes there).  Deterministic: the
 *           position slices are summed in a fixed order.
 * workspace: capamd_ngram_conv_workspace_floats(D, G, F, backward) fp32 values, 16-byte aligned (CAPAMD_ERR_WORKSPACE below that). */
size_t capamd_ngram_conv_workspace_floats(int D, int G, int F, int backward);
int capamd_ngram_conv_forward(const int64_t* q_ids, const int64_t* d_ids, int N, int Q, int L, const float* emb, int64_t V, int D,
                              const float* const* conv_w, const float* const* conv_b, int G, int F, float* qrep, float* drep,
                              float* workspace, size_t workspace_floats, int* status, void* stream);
int capamd_ngram_conv_backward(const int64_t* q_ids, const int64_t* d_ids, int N, int Q, int L, const float* emb, int64_t V, int D, int G,
                               int F, const float* dqrep, const float* ddrep, float* const* dconv_w, float* const* dconv_b,
                               float* workspace, size_t workspace_floats, int* status, void* stream);

/* One ConvKNRM training step on the device (reference ConvKNRM.py:42-77 under trainer/pytorch.py:93-108, the loss
 * reranker/common.py:96-103, torch.optim.Adam): convolutions (capamd_ngram_conv_forward) -> kernel pooling (capamd_kernel_pool_forward) ->
 * single-Linear combine (+ tanh), pairwise loss (0 hinge / 1 softmax), its backward and Adam on the Linear in ONE workgroup -> pooling
 * backward -> the partial results' reductions + Adam on the kernels' mu / sigma -> convolution weight gradients
 * (capamd_ngram_conv_backward) -> Adam on the convolutions.  Eleven launches, no autograd, no ATen node.
 * q_ids int64 [2 B, Q] (the batch's queries twice), d_ids int64 [2 B, L] (the positive documents, then the negative ones);
 * ptrs: HOST array of 3 P device pointers, P = 2 K + 2 G + 2 - kernels.kernels.{k}.mu (K), .sigma (K), convs.{g}.0.weight / .bias (G pairs),
 * combine.0.weight [K V], combine.0.bias [1], then their exp_avg, then their exp_avg_sq (null moments: a parameter that is not trained).
 * step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t) from the host (double).  loss_out: fp32 [1].  B <= 512; other limits as
 * the two kernel families'.  workspace: capamd_convknrm_train_step_workspace_floats(...) floats, 16-byte aligned. */
size_t capamd_convknrm_train_step_workspace_floats(int B, int Q, int L, int D, int G, int F, int K, int crossmatch);
int capamd_convknrm_train_step(const int64_t* q_ids, const int64_t* d_ids, int B, int Q, int L, const float* emb, int64_t V, int D, int G, int F,
                               int K, int crossmatch, float* const* ptrs, int scoretanh, int loss_type, float step_size, float one_minus_beta1,
                               float beta2, float eps, float bc2_sqrt, float* loss_out, float* workspace, size_t workspace_floats, int* status,
                               void* stream);

/* ---- differentiable kernel pooling over dense n-gram representations (ConvKNRM's training step) ---------
 * The part of ConvKNRM_class.forward between its trainable n-gram convolutions and `combine`, capreolus/reranker/ConvKNRM.py:53-76
 * (StackedSimilarityMatrix common.py:195-221 + RbfKernelBank common.py:224-250), forward and backward - so that the reference
 * trainer's loss.backward() (trainer/pytorch.py:96-107) reaches the convolutions through HIP kernels, not ATen ops.
 * qrep fp32 [B, GQ, Q, F] / drep fp32 [B, GD, L, F]: the GQ / GD n-gram views of query and document (F % 4 == 0, F <= 256);
 * q_ids / d_ids: the token ids (pad = 0: masked positions); crossmatch != 0: every (query view, document view) pair, V = GQ GD
 * views (v = gq GD + gd), else the matching ones (GQ == GD, V = GD).  (crossmatch ? GQ : 1) * Q <= 24, K <= 16.
 * A document's real positions are split into at most C = capamd_kernel_pool_chunks(L) chunks (1..8 slots; 160 real positions per chunk forward, 64 backward; unused slots hold zeros), one workgroup per
 * (pair, document view, chunk); pad positions never reach the similarity loop (a masked entry is the constant 0: a closed form).
 * forward:  feat fp32 [B, K V] (feature k V + v, the reference's kernels.reshape(B, K V, Q, L) order); ksum fp32 [B, GD, T, K] and
 *           rowsum fp32 [B, GD, T] (T = (crossmatch ? GQ : 1) Q) are what the backward needs of it; chunk_sums: B GD C T (K + 1) fp32
 *           values of scratch (the chunks' partial sums, added up in their order by a second launch).
 * backward: gfeat fp32 [B, K V] -> dq_part fp32 [B, GD, C, T, F] (the caller sums over C, and over GD the blocks that share a query
 *           view: with crossmatch view gq = t / Q of every gd; without, block gd holds query view gd), dd fp32 [B, GD, L, F] (zero
 *           rows at pad positions), dmu_part / dsigma_part fp32 [B GD C, K] (summed over their first axis by the caller). */
int capamd_kernel_pool_chunks(int L);
int capamd_kernel_pool_forward(const float* qrep, const float* drep, const int64_t* q_ids, const int64_t* d_ids, int B, int GQ, int GD, int Q,
                               int L, int F, int crossmatch, const float* mu, const float* sigma, int K, float* feat, float* ksum,
                               float* rowsum, float* chunk_sums, void* stream);
int capamd_kernel_pool_backward(const float* qrep, const float* drep, const int64_t* q_ids, const int64_t* d_ids, int B, int GQ, int GD, int Q,
                                int L, int F, int crossmatch, const float* mu, const float* sigma, int K, const float* gfeat,
                                const float* ksum, const float* rowsum, float* dq_part, float* dd, float* dmu_part, float* dsigma_part,
                                void* stream);

/* ---- PACRR's trainable convolution stage with its gradient (PACRR's training step) --------------------------
 * PACRRConvMax2dModule.forward, capreolus/reranker/PACRR.py:68-78, for every n-gram size mingram..maxgram at once: zero padding,
 * Conv2d(1 -> nfilters, ng x ng) over the similarity matrix sim fp32 [B, Q, L] (capamd_similarity_matrix), ReLU, max over the
 * filters, the kmax largest values over the document - and, for the reference trainer's loss.backward() (trainer/pytorch.py:96-107),
 * the coordinates of every value.  conv_w / conv_b as in capamd_pacrr_forward.  Q <= 8, L <= 1024, maxgram <= 3, kmax <= 4.
 * forward:  top fp32 / pos int32 / filt int32 [B, Q, n_ngrams * kmax]: value, document position, filter (-1: a ReLU zero).
 * backward: gtop fp32 [B, Q, n_ngrams * kmax] -> dconv_w, dconv_b (laid out like conv_w / conv_b; summed in a fixed order). */
int capamd_pacrr_convmax_forward(const float* sim, int B, int Q, int L, int mingram, int maxgram, int nfilters, int kmax, const float* conv_w,
                                 const float* conv_b, float* top, int32_t* pos, int32_t* filt, void* stream);
int capamd_pacrr_convmax_backward(const float* sim, int B, int Q, int L, int mingram, int maxgram, int nfilters, int kmax, const float* gtop,
                                  const int32_t* pos, const int32_t* filt, float* dconv_w, float* dconv_b, void* stream);

/* ---- ranking of scored candidate lists ---------------------------------------------
 * What follows the scoring call in the reference, kept on the device:
 *   - score.astype(np.float16)                         capreolus/trainer/pytorch.py:346-348
 *   - Searcher.write_trec_run's per-query stable sort  capreolus/searcher/__init__.py:48-58
 *   - trec_eval's ndcg_cut_k behind evaluator.py:55-85 (score desc, ties by docid desc, gain = level, log2 discount)
 * scores fp32 [total]; offsets int64 [n_queries + 1] (CSR: query q owns scores[offsets[q] .. offsets[q+1])),
 * max_candidates >= the longest list (<= 16384).
 * capamd_rank_candidates: out_idx int32 [n_queries, k] = positions inside the query's list in run-file order
 *   (rounded score descending, equal scores in list order; -1 beyond the list), out_f16 uint16 [n_queries, k] = the
 *   rounded scores' fp16 bits.
 * capamd_ndcg_cut (k <= 256): rel int32 [total] relevance level of each candidate (0 = unjudged), tie int32 [total] =
 *   the candidate's rank in docid-descending order inside its query (a permutation of 0..n-1), idcg fp64 [n_queries] =
 *   the ideal DCG@k from the query's qrels (host side); out fp64 [n_queries] = nDCG@k (0 when idcg is 0).
 * Status bits: CAPAMD_STATUS_SCORE_NAN, CAPAMD_STATUS_TIE_RANGE. */
int capamd_rank_candidates(const float* scores, const int64_t* offsets, int n_queries, int max_candidates, int k,
                           int32_t* out_idx, uint16_t* out_f16, int* status, void* stream);
int capamd_ndcg_cut(const float* scores, const int64_t* offsets, const int32_t* rel, const int32_t* tie, const double* idcg,
                    int n_queries, int max_candidates, int k, double* out, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CAPREOLUS_AMD_H */
