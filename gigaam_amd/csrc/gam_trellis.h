// gam_trellis.h -- what the sequential trellis sweeps share: gam_align.h (CTC, one workgroup per utterance), gam_align_long.h (CTC,
// one utterance tiled over states and frames) and gam_rnnt_align.h (transducer lattice by anti-diagonals).  Everything here is a
// forceinline function of plain values: the kernels keep their loops, their loads and their fp64 offsets.
//
// The renormalised sweep (all three).  A workgroup steps through the trellis with ONE barrier per step, Viterbi values d and forward
// values a double-buffered in LDS (buf = step & 1).  Every step subtracts the previous step's maximum (of d and of a separately) and
// the kernel adds what was subtracted to an fp64 offset, so the stored values stay O(one step's log-prob) and their fp32 ulp far below
// the top-1 / top-2 margins of real frames.  The maxima travel through wm: each wave publishes the maximum of what it wrote, every
// thread reads all 16 slots after the barrier.  A step whose predecessors are all unreachable subtracts 0 (the -inf -> 0 rule).
//
// The CTC rules (both CTC kernels, shared with tests/ctc_align_ref.py).  Extended labels l = (blank, y0, blank, y1, ..., blank),
// S = 2U + 1 states; state s takes s, s - 1 and, when l_s is a token that differs from l_{s-2}, s - 2.  Tie rule: among equal
// predecessors prefer s over s-1 over s-2; at the end prefer S-1 over S-2.  Backpointers: the decrement 0 / 1 / 2 as 2 bits per
// (t, s), stored as two 64-bit ballots per 64-state chunk {bit0 lo, bit0 hi, bit1 lo, bit1 hi}.  Feasible: T >= U + #{i : y_i ==
// y_{i-1}} and every id in [0, V-2].
//
// The wildcard (the STAR variants of both CTC kernels).  Target id V, one past blank, is an ordinary token in all of the above -- it
// takes a frame, blanks may flank it, two adjacent wildcards are a repeat, it counts in U -- except that its emission at frame t is
// star[t], a per-frame value of the caller's, not a column of lp.  Nothing of (b) .. (e) changes: gam_ctc_lanes compares labels and V is
// a label like any other.  What changes is where a state's emission is loaded from: gam_ctc_star_src below.
#pragma once
#include "gam_common.h"

#define GAM_ALIGN_MAX_NT 1024
#define GAM_ALIGN_MAX_SPT 3
#define GAM_ALIGN_PF 4          // emission rows in flight ahead of the step that uses them

// ------------------------------------------------------------------ (a) the renormalisation frame
#define GAM_TRELLIS_WM 64       // floats: per-wave maxima of a step, wm[(buf * 2 + {0: d, 1: a}) * 16 + wave]

__device__ __forceinline__ void gam_trellis_wm_init(float* wm, int tid) {
  if (tid < GAM_TRELLIS_WM) wm[tid] = -INFINITY;
}
// the maxima of the step that wrote `buf`: what this step subtracts and the kernel adds to its offsets
__device__ __forceinline__ void gam_trellis_wm_read(const float* wm, int buf, float& mD, float& mA) {
  mD = mA = -INFINITY;
#pragma unroll
  for (int w = 0; w < 16; w += 4) {   // (all 16 slots: those of absent waves hold -inf)
    const float4 xd = *reinterpret_cast<const float4*>(wm + (buf * 2) * 16 + w);
    const float4 xa = *reinterpret_cast<const float4*>(wm + (buf * 2 + 1) * 16 + w);
    mD = fmaxf(mD, fmaxf(fmaxf(xd.x, xd.y), fmaxf(xd.z, xd.w)));
    mA = fmaxf(mA, fmaxf(fmaxf(xa.x, xa.y), fmaxf(xa.z, xa.w)));
  }
  if (mD == -INFINITY) mD = 0.f;
  if (mA == -INFINITY) mA = 0.f;
}
// wave maximum of the threads' local maxima; lane 0 publishes it for the step that will read `buf`
__device__ __forceinline__ void gam_trellis_wm_publish(float* wm, int buf, int lane, int wave, float lmD, float lmA) {
  lmD = gam_dpp_wave_max(lmD);
  lmA = gam_dpp_wave_max(lmA);
  if (lane == 0) {
    wm[(buf * 2) * 16 + wave] = lmD;
    wm[(buf * 2 + 1) * 16 + wave] = lmA;
  }
}

// ------------------------------------------------------------------ (b) CTC: this thread's states
// Local state i * nt + tid of a block of `nloc` states that starts at global state s0 (one workgroup for all states: s0 = 0,
// nloc = S): the label, whether the state exists, whether its s-2 skip is allowed.
template <int SPT>
__device__ __forceinline__ void gam_ctc_lanes(const int* y, int blank, int S, int s0, int nloc, int nt, int tid, int (&lab)[SPT],
                                              bool (&act)[SPT], bool (&skip)[SPT]) {
#pragma unroll
  for (int i = 0; i < SPT; ++i) {
    const int sl = i * nt + tid, s = s0 + sl;
    act[i] = sl < nloc && s < S;
    const bool tok = act[i] && (s & 1);
    lab[i] = tok ? y[(s - 1) >> 1] : blank;
    skip[i] = tok && s >= 3 && y[(s - 1) >> 1] != y[(s - 3) >> 1];
  }
}

// STAR variants: where each of this thread's states reads its emission.  Frame t of a state is src[t * stride]: (lp + label, V) for a
// label or blank, (star, 1) for the wildcard label V.  One unconditional load per state and step, as without wildcards; no select and
// no scalar load on the step's chain.
template <int SPT>
__device__ __forceinline__ void gam_ctc_star_src(const float* lp, const float* star, int V, const int (&lab)[SPT], const float* (&src)[SPT],
                                                 int (&stride)[SPT]) {
#pragma unroll
  for (int i = 0; i < SPT; ++i) {
    const bool w = lab[i] == V;
    src[i] = w ? star : lp + lab[i];
    stride[i] = w ? 1 : V;
  }
}
// the bad-id rule: [0, V-2] are labels, V-1 is blank, V is the wildcard where the kernel is a STAR variant
template <bool STAR>
__device__ __forceinline__ bool gam_ctc_bad_id(int v, int V) {
  return STAR ? (v < 0 || v > V || v == V - 1) : (v < 0 || v > V - 2);
}

// ------------------------------------------------------------------ (c) CTC: one frame of one state
// Dp / Ap: the previous frame's rows, Dc / Ac: this frame's, all indexed by local state s (index -1 and -2 readable); e: the state's
// emission log-prob; mD / mA from gam_trellis_wm_read.  Returns the backpointer code; nd / na are the new values (-inf for an absent
// state), folded into the thread's local maxima lmD / lmA.  Each kernel calls it from its own unrolled loop over its SPT states: a form
// that took all SPT states and handed nd / na back as arrays cost the tiled kernel three VGPRs and a wave of occupancy at SPT = 2.
__device__ __forceinline__ unsigned gam_ctc_step(const float* Dp, const float* Ap, float* Dc, float* Ac, int s, bool act, bool skip, float e,
                                                 float mD, float mA, float& lmD, float& lmA, float& nd, float& na) {
  unsigned bp = 0;
  nd = na = -INFINITY;
  if (act) {
    const float d0 = Dp[s], d1 = Dp[s - 1], d2 = skip ? Dp[s - 2] : -INFINITY;
    float best = d0;
    if (d1 > best) { best = d1; bp = 1; }
    if (d2 > best) { best = d2; bp = 2; }
    nd = (best - mD) + e;
    const float a0 = Ap[s], a1 = Ap[s - 1], a2 = skip ? Ap[s - 2] : -INFINITY;
    const float M = fmaxf(fmaxf(a0, a1), a2);
    if (M > -INFINITY) na = ((M - mA) + gam_fast_log(gam_fast_exp(a0 - M) + gam_fast_exp(a1 - M) + gam_fast_exp(a2 - M))) + e;
    Dc[s] = nd;
    Ac[s] = na;
    lmD = fmaxf(lmD, nd);
    lmA = fmaxf(lmA, na);
  }
  return bp;
}

// ------------------------------------------------------------------ (d) CTC: backpointers
// The wave's codes of its 64 states as one chunk word, stored by the `writer` lane (lane 0 when the chunk exists); with states
// i * nt + tid, dst is chunk i * (nt / 64) + wave of the block.  (The word is formed under the branch: formed before it, it held
// four VGPRs across the branch in every lane.)
__device__ __forceinline__ void gam_ctc_bp_pack(unsigned bp, bool writer, uint4* dst) {
  const unsigned long long m1 = __ballot(bp & 1u), m2 = __ballot(bp >> 1);
  if (writer) *dst = make_uint4((unsigned)m1, (unsigned)(m1 >> 32), (unsigned)m2, (unsigned)(m2 >> 32));
}
// the decrement 0 / 1 / 2 of state s, from the word of its chunk s >> 6
__device__ __forceinline__ int gam_ctc_bp_step(uint4 w, int s) {
  const int sh = s & 31;
  const unsigned lo = (s & 32) ? w.y : w.x, hi = (s & 32) ? w.w : w.z;
  return (int)(((lo >> sh) & 1u) | (((hi >> sh) & 1u) << 1));
}

// ------------------------------------------------------------------ (e) CTC: feasibility, end rule, outputs
__device__ __forceinline__ bool gam_ctc_feasible(long long T, long long U, int repeats, int bad_id) {
  return bad_id == 0 && T >= U + repeats;
}
// The last frame's d / a of states S-1 (d1, a1) and S-2 (d2, a2; -inf when S = 1), in the caller's value type and frame of reference.
// Returns whether a finite path ends here; s = its last state, score = its d, loglik = logsumexp(a1, a2) (-inf: none).
template <typename F>
__device__ __forceinline__ bool gam_ctc_end(int S, F d1, F d2, F a1, F a2, int& s, F& score, F& loglik) {
  s = S - 1;
  score = d1;
  if (d2 > score) { score = d2; s = S - 2; }
  const F M = fmax(a1, a2);
  const bool found = score > -INFINITY;
  loglik = found && M > -INFINITY ? M + log(exp(a1 - M) + exp(a2 - M)) : -INFINITY;
  return found;
}
// Frame t < T of the path (a state per frame): returns its label and writes tok_first / tok_last where a token's run begins / ends.
template <typename P>
__device__ __forceinline__ int gam_ctc_frame_out(const P* path, int t, int T, const int* y, int blank, int* tf, int* tl) {
  const int s = path[t];
  if (!(s & 1)) return blank;
  const int u = (s - 1) >> 1;
  if (t == 0 || path[t - 1] != s) tf[u] = t;
  if (t == T - 1 || path[t + 1] != s) tl[u] = t;
  return y[u];
}
