// gam_rnnt_beam_stream.h -- gam_rnnt_beam.h's RNN-T beam search for ONE stream of any length fed in pieces (gam_op_rnnt_beam_stream).
//
// The search is gam_rb_body, the batch kernel's own text: this kernel instantiates it with STREAM = true, and every difference lies
// behind `if constexpr (STREAM)` there.  The contract is gam_rnnt_beam.h's, unchanged: the candidates, the merge in B, the theta cut,
// the origin-key tie rule, hotwords and LM per gam_search.h, the per-frame renormalisation into `off`.  The differences:
//   frames   rows 0 .. n - 1 of the call's encp [n, JH] are stream frames t_base .. t_base + n - 1; a node records the stream frame.
//   nodes    int4 {parent, token, frame, 0}: a 31-bit frame does not fit in (v << 13) | t.
//   state    the record below instead of one launch's registers and workspace.
//   rebase   the sums the renormalisation does not touch are cut back every GAM_RB_STREAM_REBASE stream frames (below).
//   results  score and logp are float64; there is no N-best.
//
// State record (caller-owned, gam_rnnt_beam_stream_bytes), in this order:
//   GamRbStreamHdr                 128 B   phase, W, S, V, H, JH, L, hw_gen, lm_gen, beam size, node count, next frame, max_frames, t0,
//                                          the fp64 off, cb_off, lm_off
//   32 x GamRbStreamEntry          80 B    A list 0, the beam: hash, len, score, hotword node, acc, committed, prefix node, slot, and with
//                                          the LM the word state, partial-word hash, lm, d, completed word id; zeros beyond the beam
//   (S + 1) W slots                        [L][h | c] | pp floats each: the predictor states.  In the record and not in the handle's
//                                          workspace, because another decode may run between two calls of the stream
//   max_frames S W nodes           16 B    the prefix trie: at most W new hypotheses per symbol step, S steps per frame
// NOT stored: the logit rows (scratch of one joint step: the handle's workspace); the A lists beyond list 0, B, the candidates and the
// free list (a call ends only when its last frame has ended, where they are dead; the free list is rebuilt from the beam's slots at
// the end of every frame and, by the same function, at the start of every call, so slot numbers do not depend on the cutting).
//
// A call: check the call against the header; load the beam into A list 0 (BEGIN: the empty hypothesis, predict(None, None) into slot 0,
// the LM state <s>); rebuild the free list; run the n frames; store the 32 entries and the header, status[0] = 1.  Nothing is stored
// to the header or the entries inside the frame loop.  END: the batch kernel's final pick (pending hotword bonus dropped, last word
// completed, </s> added) and the backtrack behind the call's last row: count, ids / frames (at most cap), score, logp.  n = 0 is legal
// with either flag, both or none.  A stream that ends without a frame gives count 0, score = logp = 0; a beam that emptied gives count 0,
// score = logp = -inf, as the batch kernel.  All state and result stores are plain per-lane stores.
//
// Rebase: the renormalisation keeps a rank's SUM O(1) but not its terms: an entry's committed hotword bonus and its LM term are plain
// fp32 sums that grow with the stream, and the score runs to minus that.  At every stream frame t > 0 that is a multiple of
// GAM_RB_STREAM_REBASE the new beam is formed with the best kept entry's committed bonus and LM term subtracted from every entry's, and
// both amounts go to the fp64 cb_off / lm_off, which `score` adds back.  Every rank moves by the same amount, so the order stands; the
// next frame's renormalisation moves the scores and `off` by the opposite amount, so logp stands.  Rebase frames are stream frames: no
// cutting moves them, and a stream whose frames hold no positive multiple of the period is the batch kernel's arithmetic throughout.
//
// Refusals (status[0] = 0, nothing else written, the record unchanged).  Without BEGIN: a record that was not begun or has ended; a
// t_base that is not the record's next frame; W / S / V / H / JH / L other than BEGIN recorded; a hotword or LM generation that has
// moved; a pool smaller than BEGIN saw.  With or without BEGIN: t_base + n - t0 > max_frames; t_base + n >= 2^31 (gam_op_rnnt_beam_stream
// fails on the host for that before any launch -- the host error is the contract of the C ABI; the kernel's clause guards its own int
// arithmetic against a launch that did not come through it).
// Limits: the batch kernel's (W <= 32, S <= 16, V <= 1025, H and JH <= 512, multiples of 16), the same LDS carve (gam_rb_lds_bytes), and
// max_frames S W < 2^31.  One workgroup of GAM_RB_NT threads.
#pragma once
#include "gam_rnnt_beam.h"

// bytes of the record in front of the node pool
static inline size_t gam_rb_stream_fixed_bytes(int W, int S, int H, int JH, int L) {
  return GAM_RB_STREAM_HDR_BYTES + gam_rb_pool(W, S) * ((size_t)L * 2 * H + JH) * sizeof(float);
}
// floats of the logit rows (the handle's scratch)
static inline size_t gam_rb_stream_ws_floats(int W, int V) { return (size_t)((W + 15) / 16) * 16 * (size_t)((V + 3) & ~3); }

struct GamRnntBeamStreamArgs {
  GamRnntBeamArgs a;     // the weights and sizes; encp [n, JH] of this call; ws = the logit rows; ids / frames [cap], counts [1] (END only)
  GamRbStreamArgs x;
};

template <bool LM>
__global__ __launch_bounds__(GAM_RB_NT) void gam_rnnt_beam_stream_kernel(GamRnntBeamStreamArgs g) {
  if (g.a.W > 16) gam_rb_body<2, LM, false, true>(g.a, g.x);
  else gam_rb_body<1, LM, false, true>(g.a, g.x);
}
