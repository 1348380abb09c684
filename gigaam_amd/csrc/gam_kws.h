// gam_kws.h -- keyword search over CTC log-probs (gam_ctc_kws / gam_op_ctc_kws): for every (utterance, keyword) pair, where the
// keyword occurs, and how well it scores against the greedy path.
//
// For utterance b with log-probs lp[t, v] (t < T = enc_len[b], blank = V-1, read as they are) and keyword y[0..U), 1 <= U <= 64:
//   emissions  c_t(v) = lp[t, v] - max_w lp[t, w]   (a log-likelihood ratio against the greedy path: <= 0, and exactly 0 in fp32
//              where v is the frame's argmax, because the subtraction is made in fp32 on the two fp32 values)
//   states     tok_i (i < U) and blk_i (i < U - 1, the blank between token i and token i + 1); no leading / trailing blank.  Each
//              state carries a value d and the start frame st of its best path; before frame 0 every state holds -inf / -1.
//   frame t    tok_i, i > 0: best of  stay tok_i, then blk_{i-1}, then tok_{i-1} (only if y_i != y_{i-1})
//              tok_0:        best of  stay tok_0, then a FRESH START (value 0, start frame t)
//              blk_i:        best of  stay blk_i, then tok_i
//              (predecessors from frame t - 1; a later candidate wins only if STRICTLY greater: the order is the tie rule)
//              d' = best + c_t(label), st' = the chosen predecessor's; -inf stays -inf with start -1.
//   outputs    E_t = d_t(tok_{U-1}), S_t = its start: the best score of an occurrence that ends at frame t, and where it starts.
// Ties are the normal case (c = 0 on every argmax frame): the rule makes `start` the earliest frame and `end` the last frame of
// the last token's run.
//
// Hits: one streaming pass over t for the frames with E_t >= min_score[k].  No candidate open: open (E_t, S_t, t).  S_t <= the
// candidate's end (overlap): replace it by (E_t, S_t, t) if E_t >= its score, else drop the frame.  Otherwise emit the candidate
// and open (E_t, S_t, t).  After the last frame emit the open candidate.  Emitted hits fill slots 0 .. max_hits - 1 in order;
// n_hits counts every emitted hit (n_hits > max_hits: the list is truncated); the slots past it hold -1 / -inf.
//
// Shape: ONE WAVE per (utterance, keyword), GAM_KWS_WAVES waves of one utterance per workgroup (their gathers hit the same
// [T, V] block in L2), lane i holds tok_i and blk_i (value + start each).  Per frame the only cross-lane traffic is lane i-1's
// two values and two starts: four DPP wave shifts (wave_shr:1; lane 0's `old` operand is the fresh start).  No LDS, no barrier:
// a wave owns its pair.  Per frame one 4-byte gather per lane (lp[b, t, y_i]), GAM_KWS_PF rows in flight, loads unconditional
// with a clamped row index (gam_align.h says why).  The frame-uniform values -- the row maximum m and c_t(blank) -- come from
// the pre-pass kernel below ({m, lp[blank] - m} per row, a workspace of the handle): a chunk of 64 rows is ONE coalesced load
// (lane j holds row t0 + j, the next chunk in flight) and v_readlane picks frame t's pair, so no scalar load sits on the chain.
// E_t / S_t leave lane U - 1 by v_readlane; every lane runs the (wave-uniform) hit pass and lane n keeps emitted hit n in
// registers (max_hits <= 64) until the sweep is over.  NO global store sits inside the frame loop of the search proper: with a
// store possibly pending hipcc waits for vmcnt(0) at every use of a gathered row (loads and stores may return out of order with
// each other on gfx9), which empties the prefetch.  The dense rows (DENSE = true, the diagnostic outputs) are kept by lane t % 64
// and stored coalesced once per 64-frame chunk, with an explicit wait behind them so that the frames of the next chunk are
// compiled as in the store-free kernel.  Values are fp32 without renormalisation: d <= 0 and only values near min_score matter.
#pragma once
#include "gam_common.h"

#define GAM_KWS_MAX_U 64         // tokens per keyword: one lane each
#define GAM_KWS_MAX_K 4096       // keywords per set
#define GAM_KWS_MAX_HITS 64      // hit slots per pair
#define GAM_KWS_MAX_T 8192
#define GAM_KWS_PF 4             // emission rows in flight ahead of the frame that uses them
#define GAM_KWS_WAVES 4          // pairs (waves) per workgroup, all of one utterance

struct GamKwsArgs {
  const float* lp;           // [B, Tp, V]
  const int* enc_len;        // [B]
  const float2* mb;          // [B, Tp] {row maximum, lp[blank] - row maximum}, rows t < enc_len[b] (gam_kws_rowmax_kernel)
  const int* kw_off;         // [K + 1]
  const int* kw_tok;         // [kw_off[K]]
  const float* kw_min;       // [K]
  int B, Tp, V, K, max_hits;
  int* hit_frames;           // [B, K, max_hits, 2]
  float* hit_score;          // [B, K, max_hits]
  int* n_hits;               // [B, K]
  float* dense_score;        // [B, K, Tp] or NULL
  int* dense_start;          // [B, K, Tp] or NULL
};

// One wave per row t < enc_len[b]: m = max_v lp[b, t, v] (coalesced reads) and the blank's emission lp[b, t, V-1] - m.
__global__ __launch_bounds__(256) void gam_kws_rowmax_kernel(const float* __restrict__ lp, const int* __restrict__ enc_len, int Tp, int V,
                                                             long rows, float2* __restrict__ mb) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int b = (int)(row / Tp), t = (int)(row - (long)b * Tp);
  if (t >= enc_len[b]) return;
  const float* p = lp + (size_t)row * V;
  float m = -INFINITY;
  for (int v = lane; v < V; v += 64) m = fmaxf(m, p[v]);
  m = gam_wave_max(m);
  if (lane == 0) mb[row] = make_float2(m, p[V - 1] - m);
}

// lane i <- lane i - 1; lane 0 keeps `fill` (DPP wave_shr:1, no bound_ctrl: a lane without a source keeps the old operand)
__device__ __forceinline__ float gam_kws_prev(float v, float fill) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ int gam_kws_prev(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false); }

template <bool DENSE>
__global__ __launch_bounds__(64 * GAM_KWS_WAVES) void gam_ctc_kws_kernel(GamKwsArgs a) {
  const int lane = threadIdx.x & 63;
  const int nkb = (a.K + GAM_KWS_WAVES - 1) / GAM_KWS_WAVES;
  const int b = blockIdx.x / nkb;
  const int k = (blockIdx.x - b * nkb) * GAM_KWS_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (k >= a.K) return;     // (no barrier anywhere below)
  const int Tp = a.Tp, V = a.V, H = a.max_hits;
  int T = a.enc_len[b];
  T = T < 0 ? 0 : (T > Tp ? Tp : T);
  const int o0 = a.kw_off[k], U = a.kw_off[k + 1] - o0;     // 1 <= U <= 64 (gam_set_keywords)
  const float thr = a.kw_min[k];
  const size_t pair = (size_t)b * a.K + k;
  int* hf = a.hit_frames + pair * H * 2;
  float* hs = a.hit_score + pair * H;
  float* de = DENSE && a.dense_score ? a.dense_score + pair * Tp : nullptr;
  int* dst = DENSE && a.dense_start ? a.dense_start + pair * Tp : nullptr;

  // lane i: tok_i and blk_i.  Lanes past the keyword gather its last token's column and hold -inf throughout.
  const int li = lane < U ? lane : U - 1;
  const int lab = a.kw_tok[o0 + li];
  const int labp = a.kw_tok[o0 + (li > 0 ? li - 1 : 0)];
  const bool tok_on = lane < U, blk_on = lane < U - 1;
  const bool from_tok = lane == 0 || lab != labp;     // (lane 0: the fresh start sits in the tok_{i-1} slot)
  float dt = -INFINITY, db = -INFINITY;
  int st = -1, sb = -1;
  // the hit pass (wave-uniform): the open candidate; lane n holds emitted hit n
  int nh = 0, cst = 0, ce = 0;
  float cs = 0.f;
  bool open = false;
  int h_st = -1, h_en = -1;
  float h_sc = -INFINITY;

  if (T > 0) {
    const float* lpb = a.lp + (size_t)b * Tp * V + lab;
    const float2* mbb = a.mb + (size_t)b * Tp;
    float2 nx = mbb[lane < T ? lane : T - 1];
    // (the first chunk's pair is waited for HERE, once: requested beside the first rows it is the youngest load at the head of the
    // frame loop, and hipcc then waits for it -- that is, for all rows but one -- at the head of every group of frames)
    __builtin_amdgcn_s_waitcnt(0x0f70);
    float e[GAM_KWS_PF];
#pragma unroll
    for (int q = 0; q < GAM_KWS_PF; ++q) {              // (in frame order, pinned: the waits of the frame loop count on it)
      e[q] = lpb[(size_t)(q < T ? q : T - 1) * V];
      __builtin_amdgcn_sched_barrier(0);
    }
    float2 cur = nx;                                    // rows t0 .. t0 + 63 of the chunk at hand, one per lane
    float eb = -INFINITY;                               // DENSE: E / S of row t0 + lane
    int ebs = -1;
    // one frame: t = t0 + jq, its gathered row in e[q] (q a constant wherever this is expanded)
    auto frame = [&](const int q, const int jq, const int t) __attribute__((always_inline)) {
      const float m = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur.x), jq));
      const float cb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur.y), jq));
      // lane i - 1 at frame t - 1 (lane 0: the fresh start, value 0 from frame t)
      const float pt = gam_kws_prev(dt, 0.f), pb = gam_kws_prev(db, -INFINITY);
      const int pst = gam_kws_prev(st, t), psb = gam_kws_prev(sb, -1);
      float best = dt;                                  // tok_i: stay, then blk_{i-1}, then tok_{i-1}
      int bs = st;
      if (pb > best) { best = pb; bs = psb; }
      if (from_tok && pt > best) { best = pt; bs = pst; }
      float bb = db;                                    // blk_i: stay, then tok_i
      int bbs = sb;
      if (dt > bb) { bb = dt; bbs = st; }
      const float ndt = tok_on ? best + (e[q] - m) : -INFINITY;
      const float ndb = blk_on ? bb + cb : -INFINITY;
      st = ndt > -INFINITY ? bs : -1;
      sb = ndb > -INFINITY ? bbs : -1;
      dt = ndt;
      db = ndb;
      // the row t + PF replaces the one just used
      const int tn = t + GAM_KWS_PF < T ? t + GAM_KWS_PF : T - 1;
      e[q] = lpb[(size_t)tn * V];
      const float E = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dt), U - 1));
      const int S = __builtin_amdgcn_readlane(st, U - 1);
      if (DENSE && lane == jq) { eb = E; ebs = S; }
      if (E >= thr) {
        if (open && S > ce) {                           // past the open candidate: emit it
          if (lane == nh) { h_st = cst; h_en = ce; h_sc = cs; }
          ++nh;
          open = false;
        }
        if (!open || E >= cs) { cs = E; cst = S; ce = t; open = true; }
      }
    };
    for (int t0 = 0; t0 < T; t0 += 64) {
      cur = nx;
      const int tn64 = t0 + 64 + lane;
      nx = mbb[tn64 < T ? tn64 : T - 1];                // the next chunk: in flight during this one
      // Whole groups of PF frames first, WITHOUT an early exit inside a group: an exit edge from the middle of a group back to the
      // loop header makes hipcc assume the row just requested may be the only load in flight there, i.e. wait for vmcnt(0).
      const int left = T - t0 < 64 ? T - t0 : 64, whole = left & ~(GAM_KWS_PF - 1);
      for (int j = 0; j < whole; j += GAM_KWS_PF) {
#pragma unroll
        for (int q = 0; q < GAM_KWS_PF; ++q) frame(q, j + q, t0 + j + q);
      }
#pragma unroll
      for (int q = 0; q < GAM_KWS_PF - 1; ++q)          // the last chunk's frames past its whole groups
        if (whole + q < left) frame(q, whole + q, t0 + whole + q);
      if (DENSE) {
        if (de != nullptr && t0 + lane < T) de[t0 + lane] = eb;
        if (dst != nullptr && t0 + lane < T) dst[t0 + lane] = ebs;
        __builtin_amdgcn_s_waitcnt(0x0f70);             // vmcnt(0): no store is pending in the frames that follow
      }
    }
    if (open) {
      if (lane == nh) { h_st = cst; h_en = ce; h_sc = cs; }
      ++nh;
    }
  }
  if (lane == 0) a.n_hits[pair] = nh;
  if (lane < H) {                   // (H <= 64: one slot per lane; lanes >= nh still hold -1 / -inf)
    hf[2 * lane] = h_st;
    hf[2 * lane + 1] = h_en;
    hs[lane] = h_sc;
  }
  for (int t = T + lane; t < Tp; t += 64) {
    if (de != nullptr) de[t] = -INFINITY;
    if (dst != nullptr) dst[t] = -1;
  }
}
