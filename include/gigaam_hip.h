/* gigaam_hip.h -- C ABI of libgigaam_hip.so: the MI355X (gfx950) inference path for
 * GigaAM's log-mel frontend, Conformer encoder and CTC / RNN-T greedy decoders.
 *
 * This is the drop-in boundary of SURVEY.md §8b.  The reference has no FFI of its own
 * (it is pure Python on torch); what it has is three operator slots instantiated from
 * the checkpoint config (reference gigaam/model.py:24-25,93-94) with plain-tensor call
 * contracts.  Each entry point below replaces exactly one of those calls and is what a
 * ctypes binding on the reference side would load (INTEGRATION.md shows the stub):
 *
 *   gam_frontend     <- FeatureExtractor.forward          gigaam/preprocess.py:94-98
 *   gam_encode       <- ConformerEncoder.forward          gigaam/encoder.py:605-647
 *   gam_ctc_head     <- CTCHead.forward                   gigaam/decoder.py:18-21
 *   gam_ctc_greedy   <- CTCGreedyDecoding.decode          gigaam/decoding.py:56-96
 *   gam_ctc_align    (no reference counterpart: CTC forced alignment + log-likelihood of a given transcript)
 *   gam_ctc_kws      (no reference counterpart: keyword search -- where each phrase of a set occurs, with a score)
 *   gam_ctc_beam     (no reference counterpart: CTC prefix beam search with hotword boosting and n-gram LM fusion)
 *   gam_ctc_beam_nbest   (no reference counterpart: the N best prefixes of that search's final beam)
 *   gam_rnnt_greedy  <- RNNTGreedyDecoding.decode         gigaam/decoding.py:128-207
 *   gam_rnnt_beam    (no reference counterpart: RNN-T beam search with hotword boosting and n-gram LM fusion)
 *                        (+ RNNTDecoder.predict decoder.py:85-102, RNNTJoint.joint :41-47)
 *   gam_rnnt_beam_nbest  (no reference counterpart: the N best hypotheses of that search's final beam)
 *   gam_emo_probs    <- GigaAMEmo.get_probs (pool+head)    gigaam/model.py:272-285
 *   gam_set_weight   <- nn.Module.load_state_dict         gigaam/__init__.py:185
 *   gam_create       <- hydra.utils.instantiate(cfg.*)    gigaam/model.py:24-25,93-94
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types.  All tensor pointers are DEVICE
 *     pointers unless the parameter says "host".  The caller owns every input/output
 *     buffer; the library owns weights, position tables and a grow-only workspace.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream) and performs no host synchronisation, except that a workspace
 *     growth (first call at a larger shape) allocates.
 *   - return value 0 = success, negative = error; gam_last_error() has the message.
 *   - one handle per device; a handle is not thread-safe; distinct handles are independent.
 *   - storage and accumulation are fp32 end to end (the parity target is the reference's
 *     fp32 CPU path); see gam_set_gemm_mode for how the dense contractions are evaluated.
 */
#ifndef GIGAAM_HIP_H
#define GIGAAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAM_ABI_VERSION 1

typedef struct gam_handle gam_handle;

enum { GAM_SUBS_CONV2D = 0, GAM_SUBS_CONV1D = 1 };
enum { GAM_ATT_ROTARY = 0, GAM_ATT_REL_POS = 1 };
enum { GAM_NORM_BATCH = 0, GAM_NORM_LAYER = 1 };
enum { GAM_HEAD_NONE = 0, GAM_HEAD_CTC = 1, GAM_HEAD_RNNT = 2, GAM_HEAD_EMO = 3 };
enum { GAM_DTYPE_F32 = 0, GAM_DTYPE_F16 = 1, GAM_DTYPE_BF16 = 2, GAM_DTYPE_F64 = 3, GAM_DTYPE_I64 = 4 };

/* POD mirror of the four cfg sub-trees of a GigaAM checkpoint. */
typedef struct gam_config {
  /* cfg.preprocessor -- FeatureExtractor(sample_rate, features, **kwargs), preprocess.py:60-65 */
  int32_t sample_rate, n_mels, hop_length, win_length, n_fft, center;
  /* cfg.encoder -- ConformerEncoder(...), encoder.py:510-526 */
  int32_t feat_in, n_layers, d_model, subsampling, subs_kernel_size, subsampling_factor;
  int32_t ff_expansion_factor, self_attention_model, n_heads, pos_emb_max_len;
  int32_t conv_norm_type, conv_kernel_size;
  /* cfg.head -- CTCHead(feat_in, num_classes) decoder.py:12-16 | RNNTHead(decoder, joint) :146-149 |
   * emotion model: a Linear(d_model, num_classes) (model.py:267-270; keys head.weight / head.bias) */
  int32_t head_type, num_classes, pred_hidden, pred_rnn_layers, joint_hidden;
} gam_config;

int gam_abi_version(void);

/* Construct the operators for one device.  Weights arrive through gam_set_weight. */
int gam_create(const gam_config* cfg, int device_id, gam_handle** out);
void gam_destroy(gam_handle* h);

/* Stage one state_dict entry (HOST pointer, copied).  `key` is the reference's
 * state_dict key ("encoder.layers.0.self_attn.linear_q.weight", ...).
 * Unknown keys are accepted and ignored (e.g. num_batches_tracked). */
int gam_set_weight(gam_handle* h, const char* key, const void* host_ptr, int dtype,
                   const int64_t* shape, int ndim);

/* Validate the key set, re-lay weights for the kernels (fused q|k|v, channels-last conv
 * taps, folded BatchNorm, DFT basis, rotary table, LSTM input table) and upload. */
int gam_finalize(gam_handle* h);

/* Shape helpers (host arithmetic): mel frames for L samples (preprocess.py:78-92) and
 * encoder frames for T mel frames (encoder.py:77-90). */
int64_t gam_feat_frames(const gam_handle* h, int64_t n_samples);
int64_t gam_enc_frames(const gam_handle* h, int64_t n_feat_frames);

/* FeatureExtractor.forward: wav f32 [B,L], len i64 [B] -> feat f32 [B,n_mels,T], feat_len i64 [B];
 * T = gam_feat_frames(L). */
int gam_frontend(gam_handle* h, const float* wav, const int64_t* wav_len, int B, int64_t L,
                 float* feat, int64_t* feat_len, void* stream);

/* ConformerEncoder.forward: feat f32 [B,feat_in,T], feat_len i64 [B] ->
 * encoded f32 [B,d_model,T'], enc_len i32 [B]; T' = gam_enc_frames(T). */
int gam_encode(gam_handle* h, const float* feat, const int64_t* feat_len, int B, int64_t T,
               float* encoded, int32_t* enc_len, void* stream);

/* Test hook: as gam_encode but stops after `n_layers_run` Conformer layers (0 = after
 * pre_encode, <0 = all) and, if tokens_out != NULL, also writes the token-major
 * activations f32 [B,T',d_model] at that point. */
int gam_encode_ex(gam_handle* h, const float* feat, const int64_t* feat_len, int B, int64_t T,
                  float* encoded, int32_t* enc_len, int n_layers_run, float* tokens_out, void* stream);

/* gam_encode / gam_encode_ex for a RAGGED batch whose lengths the caller also knows on the host (r06): feat_len_host[b] >= the device
 * value feat_len[b] (the same numbers in practice; NULL = exactly gam_encode_ex).  The Conformer layers then run on the batch's valid
 * frames only ("packed rows", gigaam_amd/csrc/gam_pack.h; the reference's counterpart is its optional flash-attn varlen attention,
 * gigaam/utils.py:103-155) instead of B x T'max rows, whenever that drops >= 3 % of the rows; outputs are the same as gam_encode's on every valid
 * frame (bit-identical at batch sizes without split-K), and frames behind an utterance's end in `encoded` are zero.  The host array is read
 * before the call returns; still no host synchronisation.  A device length above the host's is reported through the range-flag word (bit 1,
 * gam_range_flag / gam_range_flag_fetch): that batch's results are then incomplete.  n_layers_run / tokens_out as gam_encode_ex (-1, NULL). */
int gam_encode_varlen(gam_handle* h, const float* feat, const int64_t* feat_len, const int64_t* feat_len_host, int B, int64_t T,
                      float* encoded, int32_t* enc_len, int n_layers_run, float* tokens_out, void* stream);

/* Token rows the Conformer layers of the LAST gam_encode / _ex / _varlen call of this handle ran on; *rows_padded (may be NULL) = B x Ta, what
 * the padded layout takes.  Smaller than *rows_padded exactly when that call used packed rows. */
int gam_last_encode_rows(gam_handle* h, int* rows_padded);

/* CTCHead.forward: encoded f32 [B,d_model,T'] -> log_probs f32 [B,T',V]. */
int gam_ctc_head(gam_handle* h, const float* encoded, int B, int64_t Tp, float* log_probs, void* stream);

/* CTCGreedyDecoding.decode: -> ids i32 [B,T'], frames i32 [B,T'] (first counts[b] valid), counts i32 [B]. */
int gam_ctc_greedy(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp,
                   int32_t* ids, int32_t* frames, int32_t* counts, void* stream);

/* CTC forced alignment and transcript scoring (gigaam_amd/csrc/gam_align.h).  Runs the CTC head, its log-softmax and ONE alignment
 * kernel (a workgroup per utterance: Viterbi best path + forward log-likelihood in one sweep over t, backtrack in the same kernel).
 *   targets i32 [B, Umax] (entries past target_len[b] are never read), target_len i32 [B], 0 <= Umax <= 1024; blank = V - 1.
 *   frame_labels i32 [B, T']: the best path's label per frame (token id or blank), -1 at t >= enc_len[b].
 *   tok_first / tok_last i32 [B, Umax]: first / last frame of each token's run on that path, -1 past target_len[b].
 *   score f32 [B]: the best path's log-prob (sum over frames); loglik f32 [B]: log p(target | audio) = -ctc_loss.
 *   status i32 [B]: 1 aligned, 0 infeasible -- enc_len[b] < U + (adjacent repeats), a target id outside [0, V-2], target_len[b]
 *   outside [0, Umax], or no path of finite score; then score = loglik = -inf and frames / token frames are -1.
 * Ties: among equal predecessors the path keeps the state (s) over s-1 over s-2; it ends in the last token's state (S-1) over the
 * trailing blank (S-2) when both score the same.  Limits: Umax <= 1024, T' <= 8192 (an error beyond them).
 * Decode class, like gam_ctc_greedy; no host synchronisation.  Consumers of the range flag fetch it behind this call. */
int gam_ctc_align(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, const int32_t* targets,
                  const int32_t* target_len, int Umax, int32_t* frame_labels, int32_t* tok_first, int32_t* tok_last, float* score,
                  float* loglik, int32_t* status, void* stream);
/* The same from caller-supplied log-probs f32 [B, T', V] (read as they are: no normalisation), for op-level tests and callers that
 * bring their own CTC posteriors. */
int gam_op_ctc_align(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, const int32_t* targets,
                     const int32_t* target_len, int Umax, int32_t* frame_labels, int32_t* tok_first, int32_t* tok_last, float* score,
                     float* loglik, int32_t* status, void* stream);

/* CTC forced alignment of ONE long utterance (gigaam_amd/csrc/gam_align_long.h): the recurrences, tie rule, feasibility rule and
 * statuses of gam_op_ctc_align, tiled over states and frames so that the whole GPU works on it -- blocks of SB states x tiles of
 * TT frames, run as nT + nS - 1 plain launches (one per anti-diagonal) on the given stream, then a backtrack and an outputs kernel.
 *   log_probs f32 [T, V] (read as they are), targets i32 [U]; blank = V - 1.  All pointers are device pointers.
 *   frame_labels i32 [T], tok_first / tok_last i32 [U], score / loglik f64 [1] (|score| reaches 1e4-1e5 at these lengths: fp32
 *   would cost 1e-2 nats), status i32 [1]: as gam_op_ctc_align (infeasible: -inf scores, -1 everywhere; T = 0 with U = 0 scores 0).
 * Limits: T < 2^31; U whatever the workspace allows.  The workspace is the handle's: T x ceil((2U + 1) / 64) x 16 bytes of
 * backpointers + ceil((2U + 1) / SB) x T x 16 bytes of block edges + T x 4 bytes of path (+ a block row each); a call that needs
 * more than the cap fails.  Decode class; no host synchronisation (workspace growth aside). */
int gam_op_ctc_align_long(gam_handle* h, const float* log_probs, int64_t T, int V, const int32_t* targets, int U, int32_t* frame_labels,
                          int32_t* tok_first, int32_t* tok_last, double* score, double* loglik, int32_t* status, void* stream);
/* Bytes of workspace gam_op_ctc_align_long may take (0: the default, 3 GiB -- a one-hour recording, T = 9e4 frames, with a
 * char-level transcript of 5e4 tokens needs 2.25 GB of backpointers + 0.14 GB of edges; environment GAM_CTC_ALIGN_WS at gam_create). */
int gam_set_ctc_align_workspace(gam_handle* h, int64_t bytes);
/* Tuning hook of gam_op_ctc_align_long, modelled on gam_tune_sp: force the states per block (sb: a multiple of 64 in [64, 3072]) and
 * the frames per tile (tt >= 1) of every following call in this process; 0 = planned (1024 x 256).  Returns -1 for other values. */
int gam_tune_ctc_align_long(int sb, int tt);

/* Wildcard tokens: forced alignment of a PARTIAL transcript (gigaam_amd/csrc/gam_trellis.h).  In the *_star entry points target id V,
 * one past blank (= V - 1), is a wildcard: an ordinary CTC token -- at least one frame, blanks may flank it, the s - 2 skip applies
 * between it and a differing neighbour, two adjacent wildcards are a repeat, it counts in U and in T >= U + repeats -- whose emission at
 * frame t is star_lp[t] instead of a column of the log-probs.  frame_labels holds V on its frames, tok_first / tok_last its run.
 * score / loglik are those of the augmented lattice: with a wildcard, loglik is no longer the log-probability of a text.
 * Everything else -- outputs, statuses, limits, workspace cap, gam_tune_ctc_align_long, decode class, no host synchronisation -- is the
 * sibling's.  The entry points without _star keep rejecting id V.
 *   star_lp: device f32 [B, T'] (op level) / [T] (long): the emission of a wildcard state per frame, read as it is.
 * gam_op_ctc_star_row writes star_lp[b, t] = max_v log_probs[b, t, v] - penalty for t < enc_len[b] and 0 past it (enc_len NULL: every
 * row is valid; the long path calls it with B = 1, T' = T).  penalty >= 0 and finite, else an error: the greedy path's log-prob minus a
 * fixed price per frame, so a frame goes to the wildcard only where the transcript's own label is less than exp(-penalty) times as
 * likely as the frame's best label.  gam_ctc_align_star = the CTC head, its log-softmax, that row and the STAR sweep on the stream. */
int gam_op_ctc_star_row(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, float penalty,
                        float* star_lp, void* stream);
int gam_ctc_align_star(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, const int32_t* targets,
                       const int32_t* target_len, int Umax, float penalty, int32_t* frame_labels, int32_t* tok_first, int32_t* tok_last,
                       float* score, float* loglik, int32_t* status, void* stream);
int gam_op_ctc_align_star(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, const float* star_lp,
                          const int32_t* targets, const int32_t* target_len, int Umax, int32_t* frame_labels, int32_t* tok_first,
                          int32_t* tok_last, float* score, float* loglik, int32_t* status, void* stream);
int gam_op_ctc_align_long_star(gam_handle* h, const float* log_probs, int64_t T, int V, const float* star_lp, const int32_t* targets, int U,
                               int32_t* frame_labels, int32_t* tok_first, int32_t* tok_last, double* score, double* loglik,
                               int32_t* status, void* stream);

/* Windowed longform (gigaam_amd/csrc/gam_stitch.h): a long recording is cut into fixed overlapping windows that are encoded as
 * batches; the context-starved frames at each window's edges are dropped and the rest becomes ONE [T_total, V] CTC utterance.
 * gam_op_ctc_stitch copies, for every utterance b of one batch, rows lo[b] <= t < min(hi[b], enc_len[b]) of log_probs[b] to
 * out[dst[b] + t - lo[b]], bit for bit.  One call per batch writes into the same `out`.
 *   log_probs f32 [B, T', V], enc_len / lo / hi i32 [B], dst i64 [B], out f32 [T_total, V], status i32 [B]: device arrays.
 *   status[b] = 1: nothing was clipped (0 <= lo[b], hi[b] <= enc_len[b] clamped to [0, T']) and the destination rows lie inside
 *   [0, T_total), else 0.  hi[b] <= lo[b] copies nothing and is no error (status 1).  A clipped window still copies its valid rows;
 *   a window whose destination rows do not all fit copies nothing: no byte outside `out` is written.
 * Rows are V contiguous floats; accesses are 16 bytes wide where the source and the destination address allow it, 8 or 4 otherwise
 * (V = 34: rows are 8-byte aligned).  Plain vector stores, no atomics.  1 <= B <= 65535.  Decode class; no host synchronisation. */
int gam_op_ctc_stitch(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, const int32_t* lo,
                      const int32_t* hi, const int64_t* dst, float* out, int64_t T_total, int32_t* status, void* stream);
/* CTCGreedyDecoding.decode of ONE utterance of any length 0 <= T < 2^31 from caller-supplied log-probs f32 [T, V] (read as they are),
 * spread over the whole GPU: the semantics of gam_ctc_greedy's kernel -- blank = V - 1, per-frame argmax with torch's first-maximum
 * tie rule, frame t kept iff label[t] != blank && (t == 0 || label[t] != label[t - 1]), outputs in frame order -- as three plain
 * launches on the stream (labels + per-block keep counts, a scan of the block counts, compaction); no workgroup waits on another.
 *   ids / frames i32 [T] (the first count[0] entries are written), count i32 [1].  T = 0 gives count = 0.
 * 2 <= V <= 1025 (an error otherwise, without a launch).  The workspace (T + T / 128 ints at most) is the handle's.  Decode class; no host
 * synchronisation (workspace growth aside). */
int gam_op_ctc_greedy_long(gam_handle* h, const float* log_probs, int64_t T, int V, int32_t* ids, int32_t* frames, int32_t* count,
                           void* stream);

/* Keyword search over the CTC posteriors (gigaam_amd/csrc/gam_kws.h holds the contract): for every (utterance, keyword) pair, where
 * the keyword occurs and how well it scores.  Runs the CTC head, its log-softmax, a row-maximum pre-pass and ONE search kernel (a
 * wave per pair: a CTC Viterbi over the keyword's tokens with a free start and a free end, blank = V - 1).  Emissions are
 * log-likelihood ratios against the greedy path, c_t(v) = lp[t, v] - max_w lp[t, w] <= 0, so a score is 0 where the greedy path
 * spells the keyword and falls with every frame on which it does not.  Per frame t the kernel knows E_t, the best score of an
 * occurrence that ends at t, and S_t, where that occurrence starts; frames with E_t >= min_score[k] are merged into hits in one
 * streaming pass (overlapping ones keep the better, later one; gam_kws.h).  Ties follow a fixed rule: a hit starts at the earliest
 * frame and ends at the last frame of its last token's run.  Uses the set of gam_set_keywords (an error when there is none).
 *   hit_frames i32 [B, K, max_hits, 2]: (start, end) frames, end inclusive; hit_score f32 [B, K, max_hits]; in time order.
 *   n_hits i32 [B, K]: hits found; n_hits > max_hits means the list is truncated to the first max_hits.  Slots past
 *   min(n_hits, max_hits) hold -1 / -inf.  enc_len[b] = 0 gives n_hits = 0.
 *   dense_score f32 [B, K, T'] and dense_start i32 [B, K, T'] (each may be NULL): E_t and S_t; -inf / -1 where no occurrence ends
 *   and at t >= enc_len[b].
 * Limits: 1 <= max_hits <= 64, T' <= 8192 (an error beyond them, without a launch).  Decode class, like gam_ctc_greedy; no host
 * synchronisation.  Consumers of the range flag fetch it behind this call. */
int gam_ctc_kws(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, int max_hits, int32_t* hit_frames,
                float* hit_score, int32_t* n_hits, float* dense_score, int32_t* dense_start, void* stream);
/* The same from caller-supplied log-probs f32 [B, T', V] (read as they are: no normalisation). */
int gam_op_ctc_kws(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, int max_hits,
                   int32_t* hit_frames, float* hit_score, int32_t* n_hits, float* dense_score, int32_t* dense_start, void* stream);
/* The same search for ONE stream of any length fed in pieces (resumable; gam_kws.h holds the contract).  Rows 0 .. n-1 of log_probs
 * f32 [n, V] (read as they are) are stream frames t_base .. t_base + n - 1; every frame the call reports is a stream frame.  `state`
 * is a caller-owned device buffer of gam_ctc_kws_state_bytes bytes (the keyword set at hand; < 0 when there is none) that carries every
 * keyword's lattice, open candidate, hit count and next frame from call to call.  flags: GAM_KWS_STREAM_BEGIN starts a stream (the
 * state's content is ignored; n_hits = 0, all max_hits slots -1 / -inf), GAM_KWS_STREAM_END emits the open candidate behind the last
 * row and ends it; n = 0 is legal with either, both or none.  hit_frames i32 [K, max_hits, 2], hit_score f32 [K, max_hits] and n_hits
 * i32 [K] are the SAME arrays in every call of a stream: hits are written as they close, n_hits counts every one (n_hits > max_hits:
 * the list holds the first max_hits).  status i32 [K]: 1 = the call was accepted for keyword k; 0 = refused and nothing changed (the
 * state was not begun or has ended, t_base is not its next frame, or gam_set_keywords was called since BEGIN).  dense_score f32 /
 * dense_start i32 [K, n] (either may be NULL): E_t / S_t of this call's rows.  Errors without a launch: max_hits outside [1, 4096],
 * n < 0, t_base < 0, t_base + n >= 2^31, V inconsistent with the keyword ids, no keyword set, a NULL required buffer.  No host
 * synchronisation.  Decode class.
 * BUFFER SIZES ARE THE CALLER'S: every call launches one wave per keyword of the set AT HAND (K of the last gam_set_keywords), and
 * state, hit_frames, hit_score, n_hits, status and the dense rows must all be sized for that K at every call -- the library cannot
 * see their sizes.  Calling with buffers made for a set of another K is the caller's error (out-of-bounds access), not a refusal;
 * ask gam_ctc_kws_state_bytes again after every gam_set_keywords.  The device refusal covers a set of the SAME K: any successful
 * gam_set_keywords since BEGIN, an identical re-upload included, makes the state's generation stale. */
#define GAM_KWS_STREAM_BEGIN 1
#define GAM_KWS_STREAM_END 2
int64_t gam_ctc_kws_state_bytes(gam_handle* h);
int gam_op_ctc_kws_stream(gam_handle* h, const float* log_probs, int64_t n, int V, int64_t t_base, int flags, void* state, int max_hits,
                          int32_t* hit_frames, float* hit_score, int32_t* n_hits, int32_t* status, float* dense_score,
                          int32_t* dense_start, void* stream);
/* The keyword set of gam_ctc_kws: keyword i is tokens[offsets[i] .. offsets[i + 1]) (host arrays; offsets has n_keywords + 1 entries,
 * offsets[0] = 0) and reports the frames whose score reaches min_score[i] (f32 [n_keywords], finite and <= 0; U x ln(p) asks for a
 * geometric-mean likelihood ratio of p per token).  Ids outside [0, V - 2], empty keywords, more than 64 tokens in a keyword, more
 * than 4096 keywords, a non-finite or positive min_score are errors; n_keywords = 0 clears the set.  A setup call, like
 * gam_set_hotwords: it waits for the handle's in-flight decode-class work before it replaces the set. */
int gam_set_keywords(gam_handle* h, const int32_t* tokens, const int32_t* offsets, int n_keywords, const float* min_score);

/* CTC prefix beam search with hotword boosting (gigaam_amd/csrc/gam_beam.h).  Runs the CTC head, its log-softmax and ONE beam
 * kernel (a workgroup per utterance, t the sequential loop, backtrack in the same kernel).  Beam width 1 <= W <= 32; per frame the
 * top min(W, V - 1) non-blank ids are the candidate tokens; blank = V - 1.  Ties follow a fixed rule (gam_beam.h), so the result is
 * deterministic.  The hotword set of gam_set_hotwords (if any) boosts the hypotheses that spell its phrases; the n-gram LM of
 * gam_set_lm (if any) adds weight * ln P(word | history) + word_bonus for every completed word.
 *   ids / frames i32 [B, T']: the best prefix's token ids and the frame at which each token entered the beam (the first frame of its
 *   run), counts i32 [B] of them (entries past counts[b] are not written).
 *   score f32 [B]: log p of the prefix (over the paths the beam kept) + its committed hotword bonus + its LM term (every word
 *   including the last, and weight * ln P(</s> | history)); logp f32 [B]: that log p alone.
 *   enc_len[b] = 0 gives an empty result with score = logp = 0.
 * Limits: W <= 32, T' <= 8192 (an error beyond them).  Decode class, like gam_ctc_greedy; no host synchronisation. */
int gam_ctc_beam(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, int W, int32_t* ids, int32_t* frames,
                 int32_t* counts, float* score, float* logp, void* stream);
/* The same from caller-supplied log-probs f32 [B, T', V] (read as they are), 2 <= V <= 1025. */
int gam_op_ctc_beam(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, int W, int32_t* ids,
                    int32_t* frames, int32_t* counts, float* score, float* logp, void* stream);
/* The same search for ONE stream of any length fed in pieces (resumable; gam_beam_stream.h holds the contract).  Rows 0 .. n-1 of
 * log_probs f32 [n, V] (read as they are) are stream frames t_base .. t_base + n - 1; every frame the call reports is a stream frame.
 * `state` is a caller-owned device buffer (16-byte aligned) of gam_ctc_beam_stream_bytes(h, W, max_frames) bytes: the record that
 * carries the beam from call to call, and behind it the prefix-trie pool of max_frames x W nodes.  flags: GAM_BEAM_STREAM_BEGIN
 * starts a stream from the empty prefix (the state's content is ignored; with an LM the history starts at <s>), GAM_BEAM_STREAM_END
 * makes the final pick behind the call's last row (pending hotword bonus dropped, last word and </s> added), backtracks and ends the
 * stream; n = 0 is legal with either, both or none.  ids / frames i32 [max_frames], count i32 [1], score / logp f64 [1] with
 * gam_op_ctc_beam's meanings are written by the END call only; a stream that ends without a frame gives count 0, score = logp = 0.
 * One BEGIN | END call over T <= 1024 frames gives gam_op_ctc_beam's ids, frames and count, and its score and logp once rounded to
 * f32; however a stream is cut into calls, the result is the same bit for bit.  Beyond 1024 frames the committed hotword bonus and
 * the LM term are rebased into f64 offsets every 1024 stream frames (gam_beam_stream.h), so they keep their precision over hours.
 *   status i32 [1]: 1 = the call was accepted; 0 = refused and nothing else written (the state was not begun or has ended, t_base is
 *   not its next frame, W or V is not what BEGIN saw, gam_set_hotwords or gam_set_lm succeeded since BEGIN -- an identical re-upload
 *   included --, or t_base + n exceeds the frames the pool holds).
 * Errors without a launch: W outside [1, 32], V outside [2, 1025], n < 0, t_base < 0, t_base + n >= 2^31, state_bytes below the
 * record's size, a NULL required buffer, an LM whose classes are not for this V, LDS over the limit.  gam_ctc_beam_stream_bytes is
 * < 0 for W outside [1, 32], max_frames < 0 or max_frames x W >= 2^31.  Decode class; no host synchronisation. */
#define GAM_BEAM_STREAM_BEGIN 1
#define GAM_BEAM_STREAM_END 2
int64_t gam_ctc_beam_stream_bytes(gam_handle* h, int W, int64_t max_frames);
int gam_op_ctc_beam_stream(gam_handle* h, const float* log_probs, int64_t n, int V, int64_t t_base, int flags, int W, void* state,
                           int64_t state_bytes, int32_t* ids, int32_t* frames, int32_t* count, double* score, double* logp,
                           int32_t* status, void* stream);
/* N-best of the CTC prefix beam search: the same search (same kernel up to its last frame, same hotwords and LM, same limits), then
 * the N best entries of its final beam instead of the best one, 1 <= N <= W <= 32 (an error otherwise, without a launch).  An entry's
 * value is what gam_ctc_beam's final pick ranks by: log p + committed hotword bonus + LM term with the last word and </s> (a pending
 * partial hotword match does not count); order: value descending, ties to the lower beam position.
 *   ids / frames i32 [B, N, T'], counts i32 [B, N], score / logp f32 [B, N]: hypothesis r of utterance b, with gam_ctc_beam's meaning
 *   and arithmetic -- row 0 is gam_ctc_beam's result bit for bit.
 *   n_hyp i32 [B] = min(N, entries of the final beam) (prefixes of probability 0 never enter a beam, so a short utterance can have
 *   fewer than N).  Rows r >= n_hyp[b]: counts = 0, score = logp = -inf, ids / frames not written.
 *   enc_len[b] = 0 gives n_hyp = 1: one empty hypothesis with score = logp = 0.
 * The scores are the search's own (paths and alignments the beam kept), comparable within one call; gam_ctc_align scores any of the
 * hypotheses exactly.  Decode class; no host synchronisation. */
int gam_ctc_beam_nbest(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, int W, int N, int32_t* ids,
                       int32_t* frames, int32_t* counts, float* score, float* logp, int32_t* n_hyp, void* stream);
/* The same from caller-supplied log-probs f32 [B, T', V], as gam_op_ctc_beam. */
int gam_op_ctc_beam_nbest(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, int W, int N,
                          int32_t* ids, int32_t* frames, int32_t* counts, float* score, float* logp, int32_t* n_hyp, void* stream);
/* Hotword phrases for the beam search: phrase i is tokens[offsets[i] .. offsets[i + 1]) (host arrays; offsets has n_phrases + 1
 * entries, offsets[0] = 0), every matched token worth `boost` in the ranking; a partial match is rolled back when the prefix leaves
 * the phrase, and only complete phrases count in the final score.  Ids outside [0, V - 2], empty phrases, more than 1024 phrases or
 * 16384 tokens are errors; n_phrases = 0 clears the set.  A setup call, like gam_set_weight: it waits for the handle's in-flight
 * decode-class work before it replaces the set. */
int gam_set_hotwords(gam_handle* h, const int32_t* tokens, const int32_t* offsets, int n_phrases, float boost);
/* A word n-gram LM for the beam search (host arrays, copied; gigaam_amd/lm.py builds them, gam_beam.h holds the rules):
 *   token_class i32 [V] (V = the log-probs' V, blank included): 0 continues the current word, 1 starts a new word (the token belongs
 *   to it), 2 separates words (belongs to none).  A word is completed when a class-1/2 token follows a non-empty partial word.
 *   word_table: word_slots 16-byte slots {u64 key, i32 LM word id, i32 0}, keyed by the hash of the word's token ids;
 *   ngram_table: ngram_slots slots {u64 key, f32 ln p, f32 ln back-off}, keyed by the hash of the word-id tuple.  Open addressing
 *   with linear probing: slot counts are powers of two <= 2^30 (load <= 0.5 advised), word_probe / ngram_probe the longest probe
 *   chains.  order 1..5; bos / eos / unk the ids of <s>, </s>, <unk> (unk may name a word with no unigram: it then scores
 *   unk_logp).  weight (alpha) scales ln P, word_bonus (beta) is added per completed word.  ngram_slots = 0 clears the LM.
 * Token classes outside [0, 2], a bad order, slot count or probe bound are errors; a search whose V differs from the classes' is
 * an error.  A setup call: it waits for the handle's in-flight decode-class work before it replaces the tables. */
int gam_set_lm(gam_handle* h, const int32_t* token_class, int V, const void* word_table, int64_t word_slots, int word_probe,
               const void* ngram_table, int64_t ngram_slots, int ngram_probe, int order, int bos, int eos, int unk, float unk_logp,
               float weight, float word_bonus);

/* RNNTGreedyDecoding.decode: ids/frames i32 [B, T'*max_symbols], counts i32 [B].
 * Optional dump of the log-softmax of every joint evaluation, in order, per utterance:
 * logits_dump f32 [B,dump_cap,V] (may be NULL), dump_count i32 [B] (may be NULL). */
int gam_rnnt_greedy(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp,
                    int max_symbols, int32_t* ids, int32_t* frames, int32_t* counts,
                    float* logits_dump, int32_t* dump_count, int dump_cap, void* stream);
/* The encoder half of the RNN-T joint ("encp"): encoded f32 [B, d_model, T'] -> encp_out f32 [B, T', joint_hidden] = W_enc f + b_enc,
 * by the projection GEMM that gam_rnnt_greedy runs (same transpose, same GEMM arguments, same class), written to the caller's buffer:
 * what gam_op_rnnt_greedy / _beam / _align / _confidence consume.  The RNN-T twin of gam_ctc_head.  Decode class; no host
 * synchronisation. */
int gam_rnnt_encp(gam_handle* h, const float* encoded, int B, int64_t Tp, float* encp_out, void* stream);
/* gam_rnnt_greedy from a caller-supplied encp f32 [B, T', joint_hidden], the counterpart of gam_op_rnnt_beam: the same plan (the
 * cluster setting of gam_set_rnnt_cluster is honoured, the repair pass runs, gam_rnnt_last_decode is updated), no logits dump. */
int gam_op_rnnt_greedy(gam_handle* h, const float* encp, const int32_t* enc_len, int B, int64_t Tp, int max_symbols, int32_t* ids,
                       int32_t* frames, int32_t* counts, void* stream);
/* The greedy decode of ONE stream of any length fed in pieces (gigaam_amd/csrc/gam_rnnt_stream.h): one workgroup, the one-workgroup
 * kernel's frame / symbol loop, so every (frame, state) is evaluated with gam_rnnt_greedy's one-workgroup arithmetic (cluster size 0)
 * and a stream cut anywhere gives the bits of the uncut one.  Rows 0 .. n - 1 of encp f32 [n, joint_hidden] are stream frames
 * t_base .. t_base + n - 1.  state: a caller-owned record of gam_rnnt_greedy_stream_bytes(h) bytes (a header and the committed (h, c)
 * of every predictor layer) that carries the predictor from call to call.  flags: GAM_RNNT_STREAM_BEGIN starts a stream at this
 * call's t_base (any value >= 0) from predict(None, None), whatever the record held; GAM_RNNT_STREAM_END ends it.  n = 0 is legal with
 * either flag, both or none.
 *   ids / frames i32 [cap]: token k of the stream is written at index k by the call that emits it; frames are stream frames.
 *   count i32 [1]: the tokens so far, written by every accepted call -- the prefix is readable after any call.
 *   status i32 [1]: 1 = accepted; 0 = refused, nothing else written and the record unchanged.  Refused: the record was not begun or
 *   has ended (without BEGIN); t_base is not the record's next frame; max_symbols, V, pred_hidden, joint_hidden or the predictor's
 *   layers differ from what BEGIN recorded; the call could overflow cap (count + n * max_symbols > cap).  The stream carries on with the
 *   right call afterwards.
 * Errors without a launch: a head that is not RNN-T; n < 0, t_base < 0 or t_base + n >= 2^31; max_symbols < 1; cap < 0; unknown
 * flags; state_bytes below the record's size; a NULL buffer (encp may be NULL when n = 0); LDS over the limit.  Decode class; no host
 * synchronisation. */
#define GAM_RNNT_STREAM_BEGIN 1
#define GAM_RNNT_STREAM_END 2
int64_t gam_rnnt_greedy_stream_bytes(gam_handle* h);
int gam_op_rnnt_greedy_stream(gam_handle* h, const float* encp, int64_t n, int64_t t_base, int flags, int max_symbols, void* state,
                              int64_t state_bytes, int32_t* ids, int32_t* frames, int64_t cap, int32_t* count, int32_t* status,
                              void* stream);

/* RNN-T beam search with hotword boosting and n-gram LM fusion (gigaam_amd/csrc/gam_rnnt_beam.h holds the contract).  Runs the
 * encoder projection GEMM that gam_rnnt_greedy runs, then ONE beam kernel (a workgroup per utterance, t the sequential loop,
 * backtrack in the same kernel).  Beam width 1 <= W <= 32; each joint row proposes its top min(W, V - 1) non-blank ids; at most
 * max_symbols (1..16) tokens per frame, then the frame advances without a joint (greedy's rule).  Ties follow a fixed rule, so the
 * result is deterministic.  The hotword set of gam_set_hotwords (shared with the CTC search) boosts the hypotheses that spell its
 * phrases; an id >= V - 1 is an error here.  The n-gram LM of gam_set_lm (if any; shared with the CTC search) adds
 * weight * ln P(word | history) + word_bonus for every completed word, under the word rules of gam_ctc_beam; its token classes must
 * be for the model's V (an error otherwise).
 *   ids / frames i32 [B, T' * max_symbols]: the best hypothesis's token ids and the frame at which each was emitted (greedy's
 *   meaning), counts i32 [B] of them.  score f32 [B]: its log p (summed over the alignments the beam merged) + its committed hotword
 *   bonus + its LM term (every word including the last, and weight * ln P(</s> | history)); logp f32 [B]: that log p alone.
 *   enc_len[b] = 0 gives an empty result with score = logp = 0.
 * Limits: W <= 32, max_symbols <= 16, T' <= 8192, V <= 1025, pred_hidden and joint_hidden <= 512 (multiples of 16), at most 160 KiB of LDS for the
 * search state (an error beyond them; every W and max_symbols fits at pred_hidden = joint_hidden = 320 with or without the LM).
 * Decode class, like gam_rnnt_greedy; no host synchronisation. */
int gam_rnnt_beam(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, int W, int max_symbols, int32_t* ids,
                  int32_t* frames, int32_t* counts, float* score, float* logp, void* stream);
/* The beam kernel alone on a caller-supplied encoder projection encp f32 [B, T', joint_hidden] (W_enc f + b_enc), with the handle's
 * predictor and joint weights, hotwords and LM. */
int gam_op_rnnt_beam(gam_handle* h, const float* encp, const int32_t* enc_len, int B, int64_t Tp, int W, int max_symbols, int32_t* ids,
                     int32_t* frames, int32_t* counts, float* score, float* logp, void* stream);
/* The same search over ONE stream of any length fed in pieces (gigaam_amd/csrc/gam_rnnt_beam_stream.h): one workgroup, the batch
 * kernel's own search text, so a stream of fewer frames than the rebase period in one BEGIN | END call gives gam_op_rnnt_beam's bits,
 * and a stream cut anywhere gives the bits of the uncut one.  Rows 0 .. n - 1 of encp f32 [n, joint_hidden] are stream frames
 * t_base .. t_base + n - 1.  state: a caller-owned record of gam_rnnt_beam_stream_bytes(h, W, max_symbols, max_frames) bytes (a
 * header, the beam, the predictor-state slots and a prefix-trie pool of max_frames * max_symbols * W nodes of 16 bytes) that carries
 * the search -- the predictor, the hotword and the LM state of every hypothesis -- from call to call.  flags: GAM_RNNT_STREAM_BEGIN
 * starts a stream at this call's t_base (any value >= 0) from the empty hypothesis, whatever the record held; GAM_RNNT_STREAM_END
 * makes the final pick and the backtrack behind the call's rows.  n = 0 is legal with either flag, both or none.  The hotword set and
 * the LM are the handle's at BEGIN.
 *   ids / frames i32 [cap], count i32 [1], score / logp f64 [1]: written by the END call alone; at most cap tokens (the first ones),
 *   frames are stream frames; score = logp + committed bonus + LM term.  A stream without a frame: count 0, score = logp = 0.
 *   status i32 [1]: 1 = accepted; 0 = refused, nothing else written and the record unchanged.  Refused without BEGIN: the record was
 *   not begun or has ended; t_base is not the record's next frame; W, max_symbols or the head's sizes differ from what BEGIN recorded;
 *   gam_set_hotwords or gam_set_lm was called since BEGIN.  Refused with or without BEGIN: more frames since BEGIN than the record's
 *   node pool holds.  The stream carries on with the right call afterwards.
 * Errors without a launch: a head that is not RNN-T; W, max_symbols, V, pred_hidden or joint_hidden outside gam_rnnt_beam's limits;
 * n < 0, t_base < 0 or t_base + n >= 2^31; cap < 0; unknown flags; state_bytes below the record's size without nodes; a state that is not 16-byte aligned; a NULL buffer
 * (encp may be NULL when n = 0); an LM whose classes are not for this V; a hotword id >= V - 1; LDS over the limit.
 * gam_rnnt_beam_stream_bytes is < 0 outside the limits (max_frames * max_symbols * W must stay below 2^31).  Decode class; no host
 * synchronisation. */
int64_t gam_rnnt_beam_stream_bytes(gam_handle* h, int W, int max_symbols, int64_t max_frames);
int gam_op_rnnt_beam_stream(gam_handle* h, const float* encp, int64_t n, int64_t t_base, int flags, int W, int max_symbols, void* state,
                            int64_t state_bytes, int32_t* ids, int32_t* frames, int64_t cap, int32_t* count, double* score, double* logp,
                            int32_t* status, void* stream);

/* N-best of the RNN-T beam search: the same search (same kernel up to its last frame, same hotwords and LM, same limits), then the N
 * best entries of its final beam instead of the best one, 1 <= N <= W <= 32 (an error otherwise, without a launch).  An entry's value
 * is what gam_rnnt_beam's final pick ranks by: score + committed hotword bonus + LM term with the last word and </s>; order: value
 * descending, ties to the lower beam position.
 *   ids / frames i32 [B, N, T' * max_symbols], counts i32 [B, N], score / logp f32 [B, N]: hypothesis r of utterance b, with
 *   gam_rnnt_beam's meaning and arithmetic -- row 0 is gam_rnnt_beam's result bit for bit.
 *   n_hyp i32 [B] = min(N, entries of the final beam).  Rows r >= n_hyp[b]: counts = 0, score = logp = -inf, ids / frames not written.
 *   enc_len[b] = 0 gives n_hyp = 1: one empty hypothesis with score = logp = 0.
 * gam_rnnt_align scores any of the hypotheses exactly.  Decode class; no host synchronisation. */
int gam_rnnt_beam_nbest(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, int W, int max_symbols, int N,
                        int32_t* ids, int32_t* frames, int32_t* counts, float* score, float* logp, int32_t* n_hyp, void* stream);
/* The same on a caller-supplied encoder projection, as gam_op_rnnt_beam. */
int gam_op_rnnt_beam_nbest(gam_handle* h, const float* encp, const int32_t* enc_len, int B, int64_t Tp, int W, int max_symbols, int N,
                           int32_t* ids, int32_t* frames, int32_t* counts, float* score, float* logp, int32_t* n_hyp, void* stream);

/* Transducer forced alignment and transcript scoring (gigaam_amd/csrc/gam_rnnt_align.h holds the contract): the standard RNN-T
 * lattice, the one the transducer loss sums over.  For utterance b, T = enc_len[b], targets i32 [B, Umax] hold U = target_len[b]
 * token ids in [0, V - 2] (entries past U are never read), blank = V - 1.
 *   tok_frame i32 [B, Umax]: the frame at which each token is emitted on the best (Viterbi) path -- the meaning the `frames` of
 *   gam_rnnt_greedy / gam_rnnt_beam have; -1 past target_len[b].  score f32 [B]: that path's log-prob.  loglik f32 [B]:
 *   log p(targets | audio) over ALL alignments = -rnnt_loss.  (gam_rnnt_beam's logp is a lower bound of the DECODERS' capped model,
 *   where a frame advances for free after max_symbols tokens; it bounds loglik only where that cap does not bind, and can exceed it
 *   by many nats where it does.)
 *   status i32 [B]: 1 aligned (T = 0 with U = 0 included: score = loglik = 0); 0 when T = 0 with U > 0, a target id is outside
 *   [0, V - 2], target_len is outside [0, Umax] or no path has a finite score -- then score = loglik = -inf, token frames -1.
 * max_symbols_per_step does NOT bound the lattice: it is the loss's definition, not the decode's cap -- a best path may emit any
 * number of tokens in one frame and the likelihood includes such paths.  Ties: the blank predecessor wins.  Hotwords and the LM are
 * not read.  Runs the encoder projection GEMM of gam_rnnt_greedy, the teacher-forced predictor (one launch), its projection GEMM,
 * a fused joint kernel that stores only (log P(blank), log P(next token)) per lattice node, and the lattice sweep with its backtrack.
 * The lattice workspace is B x T' x (Umax + 1) x 8 bytes; above the handle's limit (gam_set_rnnt_align_workspace) the batch is
 * processed in slices of utterances with the same results; ONE utterance above the limit is an error that names the bytes.
 * Limits: Umax <= 1024, T' <= 8192, V <= 1025, pred_hidden and joint_hidden <= 512 and multiples of 16 (an error beyond them).  Decode class, like
 * gam_rnnt_greedy; no host synchronisation. */
int gam_rnnt_align(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, const int32_t* targets,
                   const int32_t* target_len, int Umax, int32_t* tok_frame, float* score, float* loglik, int32_t* status, void* stream);
/* The same from a caller-supplied encoder projection encp f32 [B, T', joint_hidden] (W_enc f + b_enc), with the handle's predictor
 * and joint weights (gam_op_rnnt_beam's counterpart).  lattice_out (may be NULL): f32 [B, T', Umax + 1, 2], a copy of the lattice
 * (log P(blank), log P(next token)) the call swept; nodes with t >= enc_len[b] or u > target_len[b] carry no defined value. */
int gam_op_rnnt_align(gam_handle* h, const float* encp, const int32_t* enc_len, int B, int64_t Tp, const int32_t* targets,
                      const int32_t* target_len, int Umax, int32_t* tok_frame, float* score, float* loglik, int32_t* status,
                      float* lattice_out, void* stream);
/* The lattice sweep alone on a caller-supplied lattice f32 [B, T', Umax + 1, 2] (read as it is; the second value at u = target_len[b]
 * is never used) for callers that bring their own joint: no model weights are needed.  targets (may be NULL: ids not checked) and V
 * only serve the id check of the status. */
int gam_op_rnnt_lattice_align(gam_handle* h, const float* lattice, const int32_t* enc_len, int B, int64_t Tp, int V, const int32_t* targets,
                              const int32_t* target_len, int Umax, int32_t* tok_frame, float* score, float* loglik, int32_t* status,
                              void* stream);
/* Bytes of lattice workspace one slice of gam_rnnt_align / gam_op_rnnt_align may take (0: the default, 1 GiB; environment
 * GAM_RNNT_ALIGN_WS sets the initial value). */
int gam_set_rnnt_align_workspace(gam_handle* h, int64_t bytes);

/* Token confidence of a finished decode (gigaam_amd/csrc/gam_confidence.h holds the contract): a post-pass over what the greedy
 * decodes, the beam searches or the alignments returned.  ids / frames i32 [B, cap] hold counts[b] tokens per utterance (their
 * decoders' meaning), blank = V - 1.  measure: 0 prob -- p(decoded token) under the step distribution it was emitted from; 1 entropy --
 * 1 - H(p) / ln V over all V classes.  Both lie in [0, 1].
 *   CTC: the step distributions are the frames of the token's span -- frames[u] and the following frames before frames[u + 1] (before
 *   enc_len[b] for the last token) whose argmax over all V classes (ties to the lower id) is ids[u]; agg combines them: 0 mean, 1 min,
 *   2 prod.  span i32 [B, cap]: the span lengths.  RNN-T: one step per token, the joint at (frames[u], ids[:u]); no span, no agg.
 *   conf f32 [B, cap]; entries past counts[b] are -1 (span 0).
 *   status i32 [B]: 1 scored (enc_len[b] = 0 with counts[b] = 0 included); 0 when an id is outside [0, V - 2], a frame is outside
 *   [0, enc_len[b]), CTC frames are not strictly increasing, RNN-T frames decrease, or counts[b] is outside [0, cap] -- then every
 *   conf is -1 and every span 0, and no entry is used as an address.
 * gam_ctc_confidence runs the CTC head, its log-softmax, ONE pass over the log-probs that keeps 8 bytes per frame (argmax, measure) in
 * a workspace of the handle, and a span walk per token.  gam_rnnt_confidence runs the encoder projection GEMM, the teacher-forced
 * predictor and its projection GEMM as gam_rnnt_align does (the decoded ids as targets), then a fused joint at the listed nodes that
 * stores one float per token; the logits never reach memory.
 * Limits (an error beyond them): V <= 1025, T' <= 8192 in these batch calls (gam_op_ctc_confidence_long takes one utterance of any
 * length); RNN-T: cap <= 1024, pred_hidden and joint_hidden <= 512 (multiples of 16).  Calling a function of
 * the other head family is an error.  Decode class; no host synchronisation. */
int gam_ctc_confidence(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, const int32_t* ids,
                       const int32_t* frames, const int32_t* counts, int cap, int measure, int agg, float* conf, int32_t* span,
                       int32_t* status, void* stream);
/* The same from caller-supplied log-probs f32 [B, T', V] (read as they are: no normalisation); needs no head. */
int gam_op_ctc_confidence(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, const int32_t* ids,
                          const int32_t* frames, const int32_t* counts, int cap, int measure, int agg, float* conf, int32_t* span,
                          int32_t* status, void* stream);
/* The CTC pass on ONE utterance of any length, 1 <= T < 2^31 (frames are int32): log_probs f32 [T, V] (read as they are), ids /
 * frames i32 [cap] and count i32 [1] on the device (a decode's or an alignment's result feeds it with no host round trip), conf f32
 * [cap], span i32 [cap], status i32 [1].  The contract above on one row with T in place of enc_len[b]: the same step distribution,
 * measures, clamp, span rule, aggregations and validity -- one bad entry anywhere in the list gives status 0, every conf -1 and every
 * span 0; count = 0 is status 1.  On a stream of at most 8192 frames conf, span and status are bit-identical to
 * gam_op_ctc_confidence with B = 1 (both run the same row pass and the same span walk).  wildcard = 1: id V (the aligners' wildcard,
 * one past blank) is a valid entry -- its frame takes part in the strictly-increasing check and bounds the previous token's span, it
 * is itself not scored (conf -1, span 0); wildcard = 0: id V is invalid.  Four launches in stream order (validity is grid-wide): a
 * memset, a check over the tokens, the row pass, one thread per token walking its span -- a token that owns N frames is walked
 * serially.  Workspace: the handle's, T x 8 bytes plus two words.  Limits (an error beyond them): 1 <= T < 2^31, 2 <= V <= 1025,
 * cap >= 0.  Needs no head.  Decode class; no host synchronisation. */
int gam_op_ctc_confidence_long(gam_handle* h, const float* log_probs, int64_t T, int V, const int32_t* ids, const int32_t* frames,
                               const int32_t* count, int cap, int measure, int agg, int wildcard, float* conf, int32_t* span,
                               int32_t* status, void* stream);
int gam_rnnt_confidence(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, const int32_t* ids,
                        const int32_t* frames, const int32_t* counts, int cap, int measure, float* conf, int32_t* status, void* stream);
/* The same from a caller-supplied encoder projection encp f32 [B, T', joint_hidden], with the handle's predictor and joint weights. */
int gam_op_rnnt_confidence(gam_handle* h, const float* encp, const int32_t* enc_len, int B, int64_t Tp, const int32_t* ids,
                           const int32_t* frames, const int32_t* counts, int cap, int measure, float* conf, int32_t* status, void* stream);

/* Workgroups per utterance of the cluster decode kernel behind gam_rnnt_greedy: -1 = as many as the device holds at once
 * (the default: the decode has the GPU to itself), 0 = the one-workgroup-per-utterance kernel, 1..8 = at most that many.
 * A caller that runs the decode of batch n on a side stream BESIDE the encoder of batch n+1 (the product's RNN-T
 * pipelines do, r05: model.launch_batch) asks for small clusters so that the latency-bound decode holds few CUs.  Every
 * setting holds the reference's bars (ids / frames / step counts exact on the fixtures, log-probs <= 1e-3; tests: C in
 * 0 .. 8) and is bit-reproducible run to run; the setting fixes how a member partitions its sums, so two
 * DIFFERENT settings may resolve a near-tie (top-1 / top-2 margin ~1e-5) differently.  gam_rnnt_greedy is safe to run
 * concurrently with gam_frontend / gam_encode of the SAME handle on another stream (it shares no scratch with them).
 * Decode-class calls of one handle (gam_ctc_head / gam_ctc_greedy / gam_rnnt_greedy / gam_rnnt_joint) share one set of
 * scratch buffers: the library orders them itself -- a call on a stream other than the previous decode-class call's first
 * waits for that call's completion event (r06) -- so the caller may put them on any streams; they never run concurrently
 * with each other.  (Environment GAM_RNNT_CLUSTER sets the initial value, clamped to -1..8.)
 * Which stream to hand over for a decode that is to run BESIDE an encoder (r06, tools/queue_probe.py): HIP maps the streams of one
 * priority level onto four hardware queues in creation order and two streams on one queue serialise -- one stream in four created with
 * hipStreamCreate shares the null stream's queue.  Create the side stream with hipStreamCreateWithPriority at the HIGH priority (its level
 * has its own queues); the Python layer does (engine.HipEngine.aux_streams). */
int gam_set_rnnt_cluster(gam_handle* h, int workgroups_per_utterance);
/* The setting in force (-1 auto, 0 .. 8); -2 for a NULL handle. */
int gam_get_rnnt_cluster(gam_handle* h);
/* What gam_rnnt_greedy's planner does with a shape (host code only: no handle, no HIP call).  ncu: the device's compute units; cluster:
 * the gam_set_rnnt_cluster setting (-1 auto); exclusive: GAM_RNNT_EXCLUSIVE; B utterances; H = pred_hidden, JH = joint_hidden, V classes,
 * L predictor layers.  out[8] = C (workgroups per utterance), NR (gate-row slots per thread), the index of the cluster kernel's
 * instantiation (0..3: H = JH = 320 at compile time; 4..8: the sizes as arguments), W_hh register-resident, the W_out slice in LDS, the
 * W_pred slice in LDS, dynamic LDS bytes of a workgroup, workgroups of the grid.  All zeros (C = 0) when the one-workgroup kernel
 * decodes the shape. */
int gam_rnnt_cluster_plan_info(int ncu, int cluster, int exclusive, int B, int H, int JH, int V, int L, int32_t* out);
/* What the LAST gam_rnnt_greedy call of this handle launched: out[3] = C used (0: the one-workgroup kernel), the index of the cluster
 * kernel's instantiation (-1 for the one-workgroup kernel), 1 if the runtime refused the cluster launch (the one-workgroup kernel then
 * decoded the batch).  Host fields; no synchronisation. */
int gam_rnnt_last_decode(gam_handle* h, int32_t* out);

/* Debug aid (r05): FNV-1a hash over one of the decode's scratch buffers as it sits in device memory (synchronises the
 * device).  which: 0 = token-major copy of the encoder output, 1 = encoder projection, 2 = hand-off granules, 3 = CTC
 * logits.  (r05's overlap investigation used it to show that nothing but the decode writes these buffers.) */
int gam_debug_buffer_hash(gam_handle* h, int which, uint64_t* hash_out, int64_t* floats_out);

/* The RNN-T head taken apart (r04): the per-step entry points the reference exposes as sub-modules.  The greedy decode above
 * never calls them; they exist for callers that drive their own search or export the head.
 * gam_rnnt_predict replaces RNNTDecoder.predict (gigaam/decoder.py:85-102) for ONE step of B samples: labels i32 [B] (a value
 * < 0 is the reference's x = None: zero embedding), h_in / c_in f32 [L, B, pred_hidden] (both NULL: zero state) ->
 * g_out f32 [B, pred_hidden] (the top layer's new hidden state = the predictor output), h_out / c_out f32 [L, B, pred_hidden].
 * gam_rnnt_joint replaces RNNTJoint.joint (gigaam/decoder.py:41-47): enc f32 [B, T, d_model], dec f32 [B, U, pred_hidden]
 * -> log_probs f32 [B, T, U, num_classes] = log_softmax(W_out relu(W_enc enc + W_pred dec)).  Exact-fp32 arithmetic. */
int gam_rnnt_predict(gam_handle* h, const int32_t* labels, const float* h_in, const float* c_in, int B, float* g_out,
                     float* h_out, float* c_out, void* stream);
int gam_rnnt_joint(gam_handle* h, const float* enc, const float* dec, int B, int T, int U, float* log_probs, void* stream);

/* GigaAMEmo.get_probs after the encoder (model.py:277-283): mean over time of encoded f32 [B,d_model,T'],
 * Linear, softmax -> probs f32 [B,num_classes].  enc_len i32 [B] restricts the mean to the valid frames of
 * each utterance; NULL = all T' frames (the reference pools its single unpadded file over the whole axis). */
int gam_emo_probs(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, float* probs,
                  void* stream);

/* Arithmetic of the dense contractions (every other kernel is plain fp32):
 *   GAM_GEMM_F32   -- v_mfma_f32_32x32x2_f32, bit-for-bit an fp32 fmaf chain.
 *   GAM_GEMM_F16X3 -- three-term split on v_mfma_f32_16x16x32_f16 with fp32 accumulation
 *                     (a = a_hi + a_lo, w = w_hi + w_lo; the a_lo.w_lo term, ~2^-22 relative,
 *                     is dropped): fp32-equivalent accuracy at several times the rate.
 *   GAM_GEMM_F16   -- OPT-IN speed mode (r04), never the default: ONE fp16 MFMA per product on plain-fp16 operands (the
 *                     producing kernels store each activation rounded once to fp16, "format 2"; the weights' hi plane;
 *                     a ~ fp16(a), w ~ fp16(w): 11 significant bits each), fp32 accumulation, fp32 softmax /
 *                     LayerNorm / residual stream -- the arithmetic contract of the reference's own GPU default (fp16
 *                     autocast + half() encoder, gigaam/model.py:34-37, gigaam/__init__.py:188-189), NOT that of its CPU
 *                     path: results differ from GAM_GEMM_F16X3 at the 1e-3 .. 1e-2 level in the encoder output.  Covers
 *                     the encoder GEMMs, the stem convolution and the attention products; the range guard below applies.
 *                     (Format 2 needs d_model and the FFN width to be multiples of 64; a model where they are only
 *                     multiples of 32 keeps the three-term GEMM kernels in this mode -- gam_encode and gam_op_gemm alike.)
 * Default: GAM_GEMM_F16X3 (environment GAM_GEMM_MODE=f32 | f16 selects another at gam_create).
 * The CTC / RNN-T head GEMMs and the windowed DFT always use GAM_GEMM_F32; gam_op_gemm follows the mode. */
enum { GAM_GEMM_F32 = 0, GAM_GEMM_F16X3 = 1, GAM_GEMM_F16 = 2 };
int gam_set_gemm_mode(gam_handle* h, int mode);
/* Range guard of GAM_GEMM_F16X3 / GAM_GEMM_F16.  LayerNorm-produced operands carry a per-row power-of-two scale and cannot leave
 * fp16's range; the other split-fp16 operands (FFN hidden, conv-module output, stem image and Conv2d#2 output, and the
 * attention's q / k / v -- its context is a convex combination of v) are split as they are, and a value beyond +-60000
 * there sets a device flag instead of silently becoming inf.  gam_range_flag copies the flag
 * accumulated since the last call to *flag_host (host int), clears it, and SYNCHRONISES `stream`; a caller that
 * sees 1 should repeat the batch under GAM_GEMM_F32 (the Python shim does).  Always 0 under GAM_GEMM_F32. */
int gam_range_flag(gam_handle* h, int* flag_host, void* stream);
/* The same without the host round trip: copies the accumulated flag into *flag_dev (a DEVICE int32) and clears it,
 * asynchronously on `stream`.  A caller that brings the decode counts to the host anyway (every transcribe path does)
 * appends one int to that buffer and reads both in ONE copy (gigaam_amd/engine.py does). */
int gam_range_flag_fetch(gam_handle* h, int32_t* flag_dev, void* stream);
int gam_get_gemm_mode(const gam_handle* h);

/* Raw GEMM entry for kernel-level tests and the roofline bench (arithmetic = current mode):
 * C[M,N] = act(A[M,K] . W[N,K]^T + bias) (act: 0 none, 1 SiLU, 2 ReLU); K % 4 == 0 (K % 32 != 0: the exact-fp32 kernel in every mode). */
int gam_op_gemm(gam_handle* h, const float* A, const float* W, const float* bias, float* C,
                int M, int N, int K, int act, void* stream);
/* Kernel-level test entry like gam_op_gemm, with the encoder's residual epilogue: C = alpha * act(A . W^T + bias) + R
 * (R f32 [M,N] dense, row pitch N, or NULL).  R is handed to the launchers as given: the split-fp16 kernel's launcher rejects
 * an R that is not 16-byte aligned (the call fails, nothing is launched); the exact-fp32 kernel reads it element-wise. */
int gam_op_gemm_ex(gam_handle* h, const float* A, const float* W, const float* bias, const float* R, float alpha,
                   float* C, int M, int N, int K, int act, void* stream);
/* The same with the encoder's output formats and range guard (split-fp16 modes only, K % 32 == 0, N % 4 == 0): C has row pitch ldc
 * elements (ldc >= N; R, when given, has the same pitch) and is written as fp32 (c_split 0), in the sp32 layout (c_split 1, ldc % 32 == 0:
 * the 4 bytes of element (row, c) hold its fp16 hi / lo pair, regrouped per 32 columns) or as plain fp16 rows (c_split 2, one-term mode
 * only, row pitch ldc halfs); c_guard != 0: a stored value beyond 60000 in magnitude sets bit 0 of the handle's range flag. */
int gam_op_gemm_fmt(gam_handle* h, const float* A, const float* W, const float* bias, const float* R, float alpha,
                    float* C, int64_t ldc, int M, int N, int K, int act, int c_split, int c_guard, void* stream);

/* Raw attention entry for kernel-level tests: q, k, v, ctx f32 [B*T, H*48] token-major
 * (head h = columns 48h..48h+47), lens i32 [B] valid keys per utterance or NULL (no mask);
 * ctx = softmax(q.k^T / sqrt(48) over keys < len).v per head (arithmetic = current mode). */
int gam_op_attention(gam_handle* h, const float* q, const float* k, const float* v, float* ctx,
                     const int32_t* lens, int B, int T, int H, void* stream);
/* Test hook: gam_op_attention with every variant the encoder launches.  q, k, v: rows of `ldq` floats (ldq >= H*48,
 * ldq % 4 == 0; q, k, v may be column offsets into one [rows, 3*H*48] buffer, as in gam_encode); ctx dense [rows, H*48].
 * Ta query rows per utterance, Tv <= Ta keys (klen_b = min(lens[b], Tv), or Tv if lens is NULL); query rows t >= klen_b
 * of a padded layout are written but carry no defined value.  cu (DEVICE i32 [B], may be NULL): packed rows -- utterance
 * b is rows cu[b] .. cu[b] + klen_b - 1 (Ta >= every klen_b: it sizes the grid); NULL = rows b*Ta .. b*Ta + Ta - 1.
 * pbuf (may be NULL) selects relative-position attention: pbuf f32 [2*Tv-1, H*48], row n = P(n - (Tv-1)), the projected
 * position embedding of relative position (query index - key index); pos_u / pos_v f32 [H*48] the two position biases:
 * score(i, j) = ((q_i + u).k_j + (q_i + v).P(i - j)) / sqrt(48). */
int gam_op_attention_ex(gam_handle* h, const float* q, const float* k, const float* v, int64_t ldq, float* ctx,
                        const int32_t* lens, const int32_t* cu, int B, int Ta, int Tv, int H, const float* pbuf,
                        const float* pos_u, const float* pos_v, void* stream);

/* Raw LayerNorm entry for kernel-level tests and microbenchmarks: every form the encoder launches (gam_norm.h), on the caller's
 * DEVICE pointers.  All float pointers 16-byte aligned; nothing is allocated.
 *   mode 0: out1 = LN(x; w1, b1).
 *   mode 1: out1 = LN(x; w1, b1) and out2 = rotary(out1): per head of dk columns (dk % 8 == 0, d % dk == 0)
 *           out2 = y cos + rotate_half(y) sin with cos / sin rows rcos / rsin f32 [rope_rows, dk/2] (the first dk/2 columns of the
 *           reference's tables) taken at frame min(t, rope_rows - 1), t = row_t[row] (i32 [rows]) or row % ta when row_t is NULL.
 *   mode 2: out1 = LN(x; w1, b1) (out1 == x allowed: the encoder's norm_out runs in place) and out2 = LN(out1; w2, b2).
 * x, out1, out2: [rows, d] dense, d % 4 == 0, d <= 1024.  split1 / split2: store format of out1 / out2 -- 0 fp32, 1 the sp32
 * split-fp16 operand layout (per 32 columns [hi x32 | lo x32] halfs in the 128 bytes of the fp32 values), 2 dense fp16 in the first
 * half of the row's bytes; 1 and 2 need d % 32 == 0.  rs (f32 [rows], may be NULL): the per-row power-of-two scale of the GEMM
 * operand -- the operand is stored multiplied by 2^e with max|row| 2^e in [2^7, 2^8) and rs[row] = 2^-e (mode 0: out1; mode 1:
 * out1 and out2 with one scale; mode 2: out2 only).
 * part (may be NULL): the fused split-K reduce -- the row is resid + palpha (sum of the nsplit slices of part [nsplit][rows][d], in
 * slice order, + pbias [d]) instead of x's; it is stored to xstore [rows, d] (modes 0 and 1; mode 2 writes it normalised to out1) and
 * then normalised.  pbias and presid [rows, d] are mandatory with part.
 * A shape the launcher refuses (d % 4, d > 1024, a split output with d % 32 != 0, dk % 8, part without bias / residual) fails with
 * a message; nothing is launched. */
typedef struct gam_ln_op {
  const float* x;
  float* out1;
  float* out2;
  const float* w1;
  const float* b1;
  const float* w2;
  const float* b2;
  const float* rcos;
  const float* rsin;
  const int32_t* row_t;
  float* rs;
  const float* part;
  const float* pbias;
  const float* presid;
  float* xstore;
  int32_t mode, rows, d, split1, split2, dk, ta, rope_rows, nsplit;
  float eps, palpha;
} gam_ln_op;
int gam_op_layernorm(gam_handle* h, const gam_ln_op* op, void* stream);

/* Raw entry of the fused conv-module middle (gam_convmod.h) for kernel-level tests and microbenchmarks:
 * z = SiLU(norm(depthwise_conv_ks(mask(GLU(u))) + dw_b)) on DEVICE pointers.  u f32 [rows, 2d] (the pointwise-conv1 output), z
 * [rows, d] in store format z_split (0 / 1 / 2 as above; 1 and 2 need d % 32 == 0), dw_w [d, ks], dw_b [d]; layer_norm = 0:
 * BatchNorm as the folded affine y n_scale + n_shift (d % 64 == 0, ks in {5, 9, 31}); 1: LayerNorm over the d channels with weight
 * n_scale and bias n_shift, eps 1e-5 (d <= 1024, ks in {5, 9, 31}).  lens i32 [B]: klen_b = min(lens[b], Tv) valid frames, frames
 * outside [0, klen_b) enter the taps as zeros whatever u holds there.  cu (i32 [B], may be NULL): packed rows -- utterance b is rows
 * cu[b] .. cu[b] + klen_b - 1 and Ta >= every klen_b sizes the grid; NULL: rows b Ta .. b Ta + Ta - 1 (Tv <= Ta), all Ta rows are
 * written and rows t >= klen_b carry no defined value.  With d % 4 == 0 the float pointers are 16-byte aligned.  A value beyond
 * +-60000 in a stored row sets the handle's range flag exactly as inside gam_encode.  Nothing is allocated. */
int gam_op_convmod(gam_handle* h, const float* u, float* z, const float* dw_w, const float* dw_b, const float* n_scale,
                   const float* n_shift, const int32_t* lens, const int32_t* cu, int B, int Ta, int Tv, int d, int ks,
                   int layer_norm, int z_split, void* stream);

/* Tuning hook of the large-M GEMM (tools/smallm_sweep.py): force the tile shape (mt in 2..4 rows of 64, nw in {2, 4}
 * columns of 64) and / or the split-K factor of every following launch in this process; 0 = planned per launch (default). */
int gam_tune_sp(int mt, int nw, int splitk);
/* The plan a launch of C[M,N] = A[M,K].W[N,K]^T would get on a device with n_cu compute units (host-side only: no GPU
 * needed; K % 32 == 0): tile rows = 64 * mt, tile columns = 64 * nw, split-K slices. */
int gam_plan_sp(int M, int N, int K, int n_cu, int* mt, int* nw, int* splitk);
/* The same with the fourth plan dimension (r04): the number of LDS stages of the kernel's operand pipeline -- 2 (the k-tile
 * after next lands while the current one is multiplied) or 3 (two k-tiles in flight: the 4-wave tiles of small grids, whose
 * k-tile is shorter than its fetch latency).  gam_tune_sp_stages forces it (0 = planned, 2, 3); tiles without a three-stage
 * build keep 2. */
int gam_plan_sp_ex(int M, int N, int K, int n_cu, int* mt, int* nw, int* splitk, int* stages);
int gam_tune_sp_stages(int stages);

/* ---- audio ingest: raw interleaved frames -> mono fp32 at another rate (gam_resample.h; handle-free like gam_plan_sp) ----------
 * Band-limited interpolation with a Hann-windowed sinc, the definition and defaults of torchaudio.functional.resample
 * (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99): with g = gcd(rate_in, rate_out), O = rate_in / g, N = rate_out / g,
 * f = 0.99 min(O, N) and x[m] = 0 outside [0, n_in),
 *     y[j] = (f / O) sum_m x[m] sinc(pi t) cos^2(pi t / 12),  t = f (m / O - j / N),  over |t| < 6,   j < n_out = ceil(N n_in / O).
 * The filter is a table of N rows (one per phase j mod N) of K taps, computed in fp64 and rounded to fp32, plus the first input
 * offset of each row: output j = q N + p reads x[first[p] + q O + k], k < K.  Equal rates are the identity (N = O = K = 1).
 *
 * gam_resample_plan    host arithmetic: *up = N, *down = O, *taps = K.  -1: a rate outside 1..384000; -2: a table of more than
 *                      2^18 entries (N K), which no call accepts.
 * gam_resample_tile    the launch a rate pair gets: outputs per workgroup, and the kernel form -- 0: N = 1 (one coefficient row,
 *                      read lane-uniformly), 1: N > 1 with the whole table in LDS, 2: N > 1 with only the tile's rows in LDS.
 * gam_resample_table   coeff f32 [N K] and first i32 [N] (HOST pointers).
 * gam_resample_out_len ceil(N n_in / O) in 64 bits; -1 for a refused rate pair.
 * gam_op_resample      src: B rows of `frames` interleaved frames of `channels` samples (DEVICE; row pitch frames * channels *
 *                      sample bytes) in format fmt; channel = -1 takes the mean of the channels (an fp32 sum in channel order times
 *                      1.0f / channels -- not a layout-aware matrix), channel = k takes channel k; the downmix precedes the filter.
 *                      len_in (device i64 [B], or NULL = every row holds `frames`): row b reads only its first len_in[b] frames, the
 *                      rest of the row counts as zeros whatever it holds.  coeff / first: the table of gam_resample_table, on the
 *                      DEVICE.  dst f32 [B, L_out]: y for j < len_out[b] = min(ceil(N len_in[b] / O), L_out), zeros up to L_out;
 *                      len_out (device i64 [B]) may be NULL.  Frame indices and byte offsets are 64-bit.  Asynchronous on `stream`;
 *                      nothing is allocated.  -1: bad argument, -2: refused rate pair, -3: the launch failed.
 * Sample formats -> fp32: u8 (v - 128) / 128; i16 v / 32768; i24 (3 bytes, little-endian) v / 8388608; i32 float(v) 2^-31; f32 as it
 * is; G.711 mu-law and A-law decoded to their 16-bit value, / 32768. */
enum { GAM_RS_FMT_U8 = 0, GAM_RS_FMT_I16 = 1, GAM_RS_FMT_I24 = 2, GAM_RS_FMT_I32 = 3, GAM_RS_FMT_F32 = 4, GAM_RS_FMT_MULAW = 5,
       GAM_RS_FMT_ALAW = 6 };
int gam_resample_plan(int rate_in, int rate_out, int* up, int* down, int* taps);
int gam_resample_tile(int rate_in, int rate_out, int* tile, int* form);
int gam_resample_table(int rate_in, int rate_out, float* coeff, int32_t* first);
int64_t gam_resample_out_len(int rate_in, int rate_out, int64_t n_in);
int gam_op_resample(const void* src, int fmt, int channels, int channel, const int64_t* len_in, int B, int64_t frames, int rate_in,
                    int rate_out, const float* coeff, const int32_t* first, float* dst, int64_t L_out, int64_t* len_out, void* stream);

/* Per-kernel-class HIP-event timing on the launch stream (bench.py's roofline leg).
 * gam_profile_enable(h,1) starts collecting for every launch, (h,2) for the GEMM family only
 * (fewer event packets inside a timed region), (h,0) stops; gam_profile_read synchronises the events and
 * returns, for class `cls`, the summed milliseconds, launch count and algorithmic work
 * (FLOP for GEMM/attention classes, bytes for the HBM-bound classes); it then resets. */
enum { GAM_PF_GEMM = 0, GAM_PF_CONV2 = 1, GAM_PF_ATTN = 2, GAM_PF_NORM = 3, GAM_PF_CONVMOD = 4,
       GAM_PF_STEM = 5, GAM_PF_FRONTEND = 6, GAM_PF_DECODE = 7, GAM_PF_MISC = 8,
       GAM_PF_ALIGN_BT = 9, GAM_PF_ALIGN_OUT = 10,   /* gam_op_ctc_align_long: its backtrack and its outputs kernel (its sweep is DECODE) */
       GAM_PF_NCLASS = 11 };
int gam_profile_enable(gam_handle* h, int on);
int gam_profile_read(gam_handle* h, int cls, double* ms, int64_t* launches, double* work);
/* Switch the collection level (0 / 1 / 2) WITHOUT resetting what was collected: bench.py samples every 4th timed step (an
 * event pair costs ~3 us on this runtime: 0.9 ms of a fully instrumented 33 ms step). */
int gam_profile_pause(gam_handle* h, int on);
/* algorithmic (unique operand + result) bytes of the timed launches of a GEMM class */
int gam_profile_read_bytes(gam_handle* h, int cls, double* bytes);

/* ---- multi-GPU: the path's ONE exchange -------------------------------------------------
 * Utterances are independent, so ranks (one process per GPU) decode disjoint shards with replicated weights
 * and never talk during the encoder; what is exchanged at the end are the fixed-shape decode buffers.  The
 * reference has no multi-device inference loop (gigaam/model.py:219-258 runs on one device); a binder that
 * shards that loop calls these three entry points.  Transport: RCCL (ncclAllGather over xGMI), resolved at
 * run time with dlopen("librccl.so.1") -- inside a torch process that is the RCCL torch already loaded.
 *
 *   gam_comm_unique_id   rank 0 makes the 128-byte RCCL id; the caller ships it to the other ranks by any
 *                        host channel it has (a file, MPI, torch.distributed's store, an environment variable)
 *   gam_comm_create      every rank: ncclCommInitRank on `device_id`
 *   gam_gather_ids       all-gather of index i32 [rows], counts i32 [rows], ids i32 [rows,cap], frames i32
 *                        [rows,cap] (DEVICE pointers; every rank passes the same rows / cap) into
 *                        all_* [world*rows ...], rank-major; one grouped RCCL call, asynchronous on `stream`.
 *                        `index` carries each row's global utterance number (or -1 for an unused row) so the
 *                        caller can restore its order; it may be NULL (then all_index must be NULL too).
 */
typedef struct gam_comm gam_comm;
#define GAM_COMM_ID_BYTES 128
int gam_comm_unique_id(char id_out[GAM_COMM_ID_BYTES]);
int gam_comm_create(const char id[GAM_COMM_ID_BYTES], int rank, int world, int device_id, gam_comm** out);
int gam_comm_world(const gam_comm* c);
int gam_gather_ids(gam_comm* c, const int32_t* index, const int32_t* counts, const int32_t* ids, const int32_t* frames,
                   int rows, int cap, int32_t* all_index, int32_t* all_counts, int32_t* all_ids, int32_t* all_frames,
                   void* stream);
const char* gam_comm_last_error(const gam_comm* c);
void gam_comm_destroy(gam_comm* c);

const char* gam_last_error(const gam_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* GIGAAM_HIP_H */
