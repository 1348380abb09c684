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
//
// A stream of any length fed in pieces, with more than 64 hits per keyword: gam_ctc_kws_stream_kernel at the end of this file (the
// same contract and the same per-frame step, gam_kws_step; the state is carried in memory and hits are flushed once per chunk).
#pragma once
#include "gam_common.h"

#define GAM_KWS_MAX_U 64         // tokens per keyword: one lane each
#define GAM_KWS_MAX_K 4096       // keywords per set
#define GAM_KWS_MAX_HITS 64      // hit slots per pair
#define GAM_KWS_MAX_T 8192
#define GAM_KWS_PF 4             // emission rows in flight ahead of the frame that uses them
#define GAM_KWS_WAVES 4          // pairs (waves) per workgroup, all of one utterance
// the resumable stream kernel (gam_ctc_kws_stream_kernel, at the end of this file)
#define GAM_KWS_STREAM_MAX_HITS 4096
#define GAM_KWS_F_BEGIN 1        // flags of a call (include/gigaam_hip.h GAM_KWS_STREAM_BEGIN / _END)
#define GAM_KWS_F_END 2
#define GAM_KWS_ST_HEAD 16       // a keyword's state record, in 4-byte words: the head, then dt | db | st | sb of the 64 lanes
#define GAM_KWS_ST_WORDS (GAM_KWS_ST_HEAD + 4 * 64)
#define GAM_KWS_ST_ACTIVE 0x4b575331     // head word 0: begun and not ended / ended; anything else is "not begun"
#define GAM_KWS_ST_ENDED 0x4b575332

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

// One wave per row t < enc_len[b] (enc_len NULL: t < Tp): m = max_v lp[b, t, v] (coalesced reads) and the blank's emission lp[b, t, V-1] - m.
__global__ __launch_bounds__(256) void gam_kws_rowmax_kernel(const float* __restrict__ lp, const int* __restrict__ enc_len, int Tp, int V,
                                                             long rows, float2* __restrict__ mb) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int b = (int)(row / Tp), t = (int)(row - (long)b * Tp);
  if (enc_len != nullptr && t >= enc_len[b]) return;     // (NULL: every row counts -- the stream kernel's calls)
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

// ONE frame of the search, shared by the batch kernel and the stream kernel below (so that the two cannot drift): lane i's tok_i /
// blk_i from frame t - 1 to frame t.  e: the lane's gathered lp[t, y_i]; m, cb: the row maximum and the blank's emission.
__device__ __forceinline__ void gam_kws_step(float& dt, float& db, int& st, int& sb, const int t, const float e, const float m,
                                             const float cb, const bool tok_on, const bool blk_on, const bool from_tok) {
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
  const float ndt = tok_on ? best + (e - m) : -INFINITY;
  const float ndb = blk_on ? bb + cb : -INFINITY;
  st = ndt > -INFINITY ? bs : -1;
  sb = ndb > -INFINITY ? bbs : -1;
  dt = ndt;
  db = ndb;
}

// The streaming hit rule on frame t's (E, S) (wave-uniform): a candidate that closes is parked in lane `slot`'s registers, ++slot.
// The stream kernel's; the batch kernel keeps the same eight lines as its own text (called from there this function moved that
// kernel from 50 to 52 SGPRs), and tests/test_hip_kws_stream.py compares the two kernels bit for bit.
__device__ __forceinline__ void gam_kws_hit(const float E, const int S, const int t, const float thr, const int lane, int& slot,
                                            bool& open, float& cs, int& cst, int& ce, int& h_st, int& h_en, float& h_sc) {
  if (E >= thr) {
    if (open && S > ce) {                           // past the open candidate: emit it
      if (lane == slot) { h_st = cst; h_en = ce; h_sc = cs; }
      ++slot;
      open = false;
    }
    if (!open || E >= cs) { cs = E; cst = S; ce = t; open = true; }
  }
}

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
      gam_kws_step(dt, db, st, sb, t, e[q], m, cb, tok_on, blk_on, from_tok);
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

// ---- The same search for ONE stream (B = 1) fed in pieces: gam_op_ctc_kws_stream.  Rows 0 .. n-1 of a call are stream frames
// t_base .. t_base + n - 1 (int32: t_base + n < 2^31); addressing uses the local row, every start frame (st, sb, the fresh start,
// S_t, the hits) the stream frame.  One wave per keyword as above, the same step (gam_kws_step), the same GAM_KWS_PF rows in flight,
// the same 64-row {m, c_blank} chunks.  What differs:
//   carry   a keyword's state record (GAM_KWS_ST_WORDS words of a caller-owned buffer): head = {phase, next frame, K, generation of
//           gam_set_keywords, hits emitted, open, cst, ce, cs} and the lanes' dt | db | st | sb.  Loaded before the first frame of a
//           call, stored after the last; nothing is stored to it inside the frame loop.
//   flush   a hit that closes is parked in lane registers (lane c holds the c-th hit closed in the 64-frame chunk at hand: a chunk
//           closes at most 64).  At the end of a chunk, if any closed, they go to slots nh .. of hit_frames / hit_score while the slot
//           is below max_hits: a wave-uniform branch, once per chunk, with an explicit vmcnt(0) behind the stores (as the dense rows
//           above), so that the frames that follow are compiled as in a store-free loop.
//   flags   BEGIN: start from -inf / -1, no candidate, no hit, whatever the state holds; n_hits = 0 and all max_hits slots -1 / -inf.
//           END: emit the open candidate behind the last row.  n = 0 is legal with either, both or none.
//   status  1: accepted.  0: refused -- the state is not begun or already ended, t_base is not its next frame, or the keyword set
//           (K, generation) is not the one it was begun with -- and NOTHING else is written.
struct GamKwsStreamArgs {
  const float* lp;           // [n, V]
  const float2* mb;          // [n] (gam_kws_rowmax_kernel with B = 1, T' = n, enc_len NULL)
  const int* kw_off;         // [K + 1]
  const int* kw_tok;
  const float* kw_min;       // [K]
  int n, V, K, max_hits, t_base, flags, gen;
  int* state;                // [K, GAM_KWS_ST_WORDS]
  int* hit_frames;           // [K, max_hits, 2]
  float* hit_score;          // [K, max_hits]
  int* n_hits;               // [K]
  int* status;               // [K]
  float* dense_score;        // [K, n] or NULL
  int* dense_start;          // [K, n] or NULL
};

template <bool DENSE>
__global__ __launch_bounds__(64 * GAM_KWS_WAVES) void gam_ctc_kws_stream_kernel(GamKwsStreamArgs a) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * GAM_KWS_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (k >= a.K) return;     // (no barrier anywhere below)
  const int n = a.n, V = a.V, H = a.max_hits, tb = a.t_base;
  int* sh = a.state + (size_t)k * GAM_KWS_ST_WORDS;
  int* sl = sh + GAM_KWS_ST_HEAD + lane;
  const bool begin = (a.flags & GAM_KWS_F_BEGIN) != 0;
  int* hf = a.hit_frames + (size_t)k * H * 2;
  float* hs = a.hit_score + (size_t)k * H;

  float dt = -INFINITY, db = -INFINITY;
  int st = -1, sb = -1;
  int nh = 0, cst = 0, ce = 0;      // the hit pass (wave-uniform): hits emitted so far and the open candidate
  float cs = 0.f;
  bool open = false;
  if (begin) {
    if (lane == 0) a.n_hits[k] = 0;
    for (int i = lane; i < H; i += 64) {
      hf[2 * i] = -1;
      hf[2 * i + 1] = -1;
      hs[i] = -INFINITY;
    }
  } else {
    const int hv = sh[lane < GAM_KWS_ST_HEAD ? lane : 0];      // the head: one word per lane
    const int phase = __builtin_amdgcn_readlane(hv, 0), next = __builtin_amdgcn_readlane(hv, 1);
    if (phase != GAM_KWS_ST_ACTIVE || next != tb || __builtin_amdgcn_readlane(hv, 2) != a.K ||
        __builtin_amdgcn_readlane(hv, 3) != a.gen) {
      if (lane == 0) a.status[k] = 0;
      return;
    }
    nh = __builtin_amdgcn_readlane(hv, 4);
    open = __builtin_amdgcn_readlane(hv, 5) != 0;
    cst = __builtin_amdgcn_readlane(hv, 6);
    ce = __builtin_amdgcn_readlane(hv, 7);
    cs = __int_as_float(__builtin_amdgcn_readlane(hv, 8));
    dt = __int_as_float(sl[0]);
    db = __int_as_float(sl[64]);
    st = sl[128];
    sb = sl[192];
  }

  if (n > 0) {
    const int o0 = a.kw_off[k], U = a.kw_off[k + 1] - o0;     // 1 <= U <= 64 (gam_set_keywords)
    const float thr = a.kw_min[k];
    float* de = DENSE && a.dense_score ? a.dense_score + (size_t)k * n : nullptr;
    int* dst = DENSE && a.dense_start ? a.dense_start + (size_t)k * n : nullptr;
    const int li = lane < U ? lane : U - 1;
    const int lab = a.kw_tok[o0 + li];
    const int labp = a.kw_tok[o0 + (li > 0 ? li - 1 : 0)];
    const bool tok_on = lane < U, blk_on = lane < U - 1;
    const bool from_tok = lane == 0 || lab != labp;
    int h_st = -1, h_en = -1;       // lane c: the c-th hit closed in the chunk at hand
    float h_sc = -INFINITY;
    const float* lpb = a.lp + lab;
    const float2* mbb = a.mb;
    float2 nx = mbb[lane < n ? lane : n - 1];
    // (as above: the first chunk's pair is waited for here, once -- and with it the state's loads and BEGIN's stores)
    __builtin_amdgcn_s_waitcnt(0x0f70);
    float e[GAM_KWS_PF];
#pragma unroll
    for (int q = 0; q < GAM_KWS_PF; ++q) {
      e[q] = lpb[(size_t)(q < n ? q : n - 1) * V];
      __builtin_amdgcn_sched_barrier(0);
    }
    float2 cur = nx;
    float eb = -INFINITY;
    int ebs = -1;
    int nc = 0;                     // hits closed in the chunk at hand
    // one frame: local row r = r0 + jq, stream frame tb + r
    auto frame = [&](const int q, const int jq, const int r) __attribute__((always_inline)) {
      const float m = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur.x), jq));
      const float cb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur.y), jq));
      const int t = tb + r;
      gam_kws_step(dt, db, st, sb, t, e[q], m, cb, tok_on, blk_on, from_tok);
      const int rn = r + GAM_KWS_PF < n ? r + GAM_KWS_PF : n - 1;
      e[q] = lpb[(size_t)rn * V];
      const float E = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dt), U - 1));
      const int S = __builtin_amdgcn_readlane(st, U - 1);
      if (DENSE && lane == jq) { eb = E; ebs = S; }
      gam_kws_hit(E, S, t, thr, lane, nc, open, cs, cst, ce, h_st, h_en, h_sc);
    };
    for (int r0 = 0; r0 < n; r0 += 64) {
      cur = nx;
      const int rn64 = r0 + 64 + lane;
      nx = mbb[rn64 < n ? rn64 : n - 1];
      const int left = n - r0 < 64 ? n - r0 : 64, whole = left & ~(GAM_KWS_PF - 1);
      for (int j = 0; j < whole; j += GAM_KWS_PF) {
#pragma unroll
        for (int q = 0; q < GAM_KWS_PF; ++q) frame(q, j + q, r0 + j + q);
      }
#pragma unroll
      for (int q = 0; q < GAM_KWS_PF - 1; ++q)
        if (whole + q < left) frame(q, whole + q, r0 + whole + q);
      if (DENSE) {
        if (de != nullptr && r0 + lane < n) de[r0 + lane] = eb;
        if (dst != nullptr && r0 + lane < n) dst[r0 + lane] = ebs;
      }
      if (nc > 0) {                 // the flush (wave-uniform): slots nh .. nh + nc - 1, those below max_hits
        const int slot = nh + lane;
        if (lane < nc && slot < H) {
          hf[2 * slot] = h_st;
          hf[2 * slot + 1] = h_en;
          hs[slot] = h_sc;
        }
        nh += nc;
        nc = 0;
        __builtin_amdgcn_s_waitcnt(0x0f70);             // vmcnt(0): no store is pending in the frames that follow
      } else if (DENSE) {
        __builtin_amdgcn_s_waitcnt(0x0f70);
      }
    }
  }
  int phase = GAM_KWS_ST_ACTIVE;
  if (a.flags & GAM_KWS_F_END) {
    if (open) {
      if (lane == 0 && nh < H) {
        hf[2 * nh] = cst;
        hf[2 * nh + 1] = ce;
        hs[nh] = cs;
      }
      ++nh;
      open = false;
    }
    phase = GAM_KWS_ST_ENDED;
  }
  // the state: the head by its first nine lanes, one word each, then the lanes' values
  int hv = phase;
  hv = lane == 1 ? tb + n : hv;
  hv = lane == 2 ? a.K : hv;
  hv = lane == 3 ? a.gen : hv;
  hv = lane == 4 ? nh : hv;
  hv = lane == 5 ? (open ? 1 : 0) : hv;
  hv = lane == 6 ? cst : hv;
  hv = lane == 7 ? ce : hv;
  hv = lane == 8 ? __float_as_int(cs) : hv;
  if (lane < 9) sh[lane] = hv;
  sl[0] = __float_as_int(dt);
  sl[64] = __float_as_int(db);
  sl[128] = st;
  sl[192] = sb;
  if (lane == 0) {
    a.n_hits[k] = nh;
    a.status[k] = 1;
  }
}
