// gam_confidence.h -- token confidence of a finished decode (gam_ctc_confidence / gam_op_ctc_confidence / gam_op_ctc_confidence_long /
// gam_rnnt_confidence / gam_op_rnnt_confidence).  A post-pass: it reads what the decoders and the alignments returned and changes none
// of their kernels.
//
// The contract (shared with tests/confidence_ref.py, float64).  For utterance b: T = enc_len[b], U = counts[b] decoded tokens
// ids[0..U) at frames[0..U) (the meaning the greedy decodes, the beam searches and the alignments give them), blank = V - 1.
//   Step distribution.  CTC: p_f = exp(lp[f, :]) over all V classes of frame f.  RNN-T, token u:
//   p = softmax(W_out relu(encp[frames[u]] + pp(y[:u])) + b_out), node (frames[u], u) of gam_rnnt_align.h's lattice: the
//   distribution the token was emitted from.
//   Measure.  prob (0): p(decoded token).  entropy (1): 1 - H(p) / ln V, H = -sum_v p_v ln p_v (p_v = 0 adds 0; V counts the
//   blank).  Both are clamped into [0, 1].
//   CTC span.  Token u owns frames[u] and every following frame f < frames[u + 1] (< T for the last token) as long as the argmax
//   of lp[f, :] over all V classes (ties to the lower id, on the fp32 values as stored) is ids[u]; frames[u] itself always belongs.
//   Its confidence is the mean (0), min (1) or product (2) of the measure over the span; the span length is an output.  An RNN-T
//   token has one step and no span.
//   Validity.  An id outside [0, V - 2], a frame outside [0, T), CTC frames not strictly increasing, RNN-T frames decreasing, or
//   counts[b] outside [0, cap]: status 0, every confidence -1, every span 0, and no entry of ids / frames decides an address.
//   Entries past counts[b] are -1 / 0.  T = 0 with U = 0 is status 1.
//
// CTC, two kernels.  gam_ctc_conf_stats_kernel reads each log-prob row ONCE: a frame is spread over a wave (V > 64) or over one
// 16-lane DPP row (V <= 64: four frames per wave), the argmax is the maximum of the key (ordered value | ~id) and sum p ln p a DPP
// sum; 8 bytes per frame -- (argmax id, the frame's measure: exp(max) or 1 - H / ln V) -- go to a workspace the handle owns
// (B x T' x 8 B).  gam_ctc_conf_agg_kernel (a workgroup per utterance) checks the rows, then one thread per token walks its span
// over those 8-byte records; only the entry frame of `prob` reads lp again (one float: its argmax may be another class).
// RNN-T.  The teacher-forced predictor and the pp GEMM of gam_rnnt_align.h with the decoded ids as targets, then
// gam_rnnt_conf_nodes_kernel: ONE WAVE takes 16 tokens of one utterance, gathers encp[b, frames[u]] + pp[b, u], keeps
// z = relu(.) in LDS (16 x JH) as the MFMA's A operand (v_mfma_f32_16x16x4_f32, exact fp32 products), streams W_out from L2 once
// (GAM_CF_NV class tiles in flight, the next k-step prefetched) and carries per node an online
// (m, S = sum e^(l - m), A = sum e^(l - m) l): H = m + ln S - A / S, ln p(token) = l_token - m - ln S.  One float per token is
// stored; the logits never reach memory and no [nodes, V] buffer exists.
// Limits (host errors): V <= 1025; the batch ops T' <= 8192 (gam_op_ctc_confidence_long below: one utterance, 1 <= T < 2^31); RNN-T:
// cap <= 1024 tokens per utterance, pred_hidden and joint_hidden <= 512 (multiples of 16; the pp GEMM takes any such K).
#pragma once
#include "gam_rnnt_align.h"

#define GAM_CF_PROB 0
#define GAM_CF_ENTROPY 1
#define GAM_CF_MEAN 0
#define GAM_CF_MIN 1
#define GAM_CF_PROD 2
#define GAM_CF_MAX_T 8192
#define GAM_CF_MAX_V 1025
#define GAM_CF_NV 4             // class tiles of the node kernel in flight

// Sums by DPP, the pattern of gam_dpp_wave_max.  Lanes a step does not write receive 0 (not their own value: that would double it).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float gam_conf_dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float gam_conf_row_sum(float v) {     // every lane: the sum of its 16-lane row
  v = gam_conf_dpp_add<0xb1, 0xf>(v);
  v = gam_conf_dpp_add<0x4e, 0xf>(v);
  v = gam_conf_dpp_add<0x141, 0xf>(v);
  return gam_conf_dpp_add<0x140, 0xf>(v);
}
__device__ __forceinline__ float gam_conf_wave_sum(float v) {    // uniform: the sum of the wave
  v = gam_conf_row_sum(v);
  v = gam_conf_dpp_add<0x142, 0xa>(v);
  v = gam_conf_dpp_add<0x143, 0xc>(v);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float gam_conf_row_max(float v) {     // every lane: the maximum of its 16-lane row
  v = gam_dpp_max<0xb1, 0xf>(v);
  v = gam_dpp_max<0x4e, 0xf>(v);
  v = gam_dpp_max<0x141, 0xf>(v);
  return gam_dpp_max<0x140, 0xf>(v);
}
__device__ __forceinline__ unsigned long long gam_conf_row_max(unsigned long long v) {
  v = gam_beam_dpp_max<0xb1, 0xf>(v);
  v = gam_beam_dpp_max<0x4e, 0xf>(v);
  v = gam_beam_dpp_max<0x141, 0xf>(v);
  return gam_beam_dpp_max<0x140, 0xf>(v);
}
__device__ __forceinline__ float gam_conf_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// ------------------------------------------------------------------ CTC 1: per-frame (argmax, measure)
struct GamConfStatArgs {
  const float* lp;         // [B, Tp, V]
  const int* enc_len;      // [B]
  int2* stats;             // [B, Tp] (argmax id, measure as f32 bits); frames t >= T are not written
  int rows, Tp, V, measure;
  float inv_lnv;           // 1 / ln V
};

template <int LPF>   // lanes per frame: 64 (a wave) or 16 (a DPP row)
__global__ __launch_bounds__(256) void gam_ctc_conf_stats_kernel(GamConfStatArgs a) {
  constexpr int FPW = 64 / LPF;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & (LPF - 1);
  const long row = ((long)blockIdx.x * 4 + wave) * FPW + lane / LPF;
  bool active = row < a.rows;
  if (active) {
    const int b = (int)(row / a.Tp);
    int T = a.enc_len[b];
    T = T > a.Tp ? a.Tp : T;
    active = (int)(row - (long)b * a.Tp) < T;
  }
  // an inactive frame loads nothing and joins the reductions with empty values (every lane runs the DPP steps)
  const float* xr = a.lp + (size_t)(active ? row : 0) * a.V;
  const int vlim = active ? a.V : 0;
  unsigned long long key = 0;
  float sum = 0.f;
  for (int v = li; v < vlim; v += LPF) {
    const float x = xr[v] + 0.0f;     // (-0 -> +0: the key orders bit patterns)
    const unsigned long long k = ((unsigned long long)gam_beam_ord(x) << 32) | (unsigned)(0xffffffffu - (unsigned)v);
    key = k > key ? k : key;          // equal values: the lower id holds the larger key
    if (a.measure == GAM_CF_ENTROPY) {
      const float p = gam_fast_exp(x);
      sum += p > 0.f ? p * x : 0.f;
    }
  }
  if (LPF == 64) {
    key = gam_beam_wave_max(key);
    sum = gam_conf_wave_sum(sum);
  } else {
    key = gam_conf_row_max(key);
    sum = gam_conf_row_sum(sum);
  }
  if (active && li == 0) {
    const int am = (int)(0xffffffffu - (unsigned)key);
    const float st = a.measure == GAM_CF_ENTROPY ? 1.0f + sum * a.inv_lnv : gam_fast_exp(gam_beam_unord((unsigned)(key >> 32)));
    a.stats[row] = make_int2(am, __float_as_int(gam_conf_clamp01(st)));
  }
}

// ------------------------------------------------------------------ CTC 2: rows checked, spans walked
struct GamConfAggArgs {
  const float* lp;         // [B, Tp, V]
  const int2* stats;       // [B, Tp]
  const int* enc_len;      // [B]
  const int* ids;          // [B, cap]
  const int* frames;       // [B, cap]
  const int* counts;       // [B]
  int Tp, V, cap, measure, agg;
  float* conf;             // [B, cap]
  int* span;               // [B, cap]
  int* status;             // [B]
};

// Token `id` entered at frame f0 of ONE utterance (lp [T, V], st [T]); the next token's frame, or T, is `lim`: its confidence, and in `n`
// the frames of its span.  The one span walk of both aggregation kernels (the same statements in the same order: the same bits).
__device__ __forceinline__ float gam_ctc_conf_span(const float* lp, const int2* st, int V, int measure, int agg, int id, int f0, int lim,
                                                   int& n_out) {
  float acc = measure == GAM_CF_PROB ? gam_conf_clamp01(gam_fast_exp(lp[(size_t)f0 * V + id])) : __int_as_float(st[f0].y);
  int n = 1;
  for (int f = f0 + 1; f < lim; ++f, ++n) {
    const int2 s = st[f];
    if (s.x != id) break;
    const float x = __int_as_float(s.y);
    acc = agg == GAM_CF_MEAN ? acc + x : (agg == GAM_CF_MIN ? fminf(acc, x) : acc * x);
  }
  n_out = n;
  return agg == GAM_CF_MEAN ? acc / (float)n : acc;
}

__global__ __launch_bounds__(256) void gam_ctc_conf_agg_kernel(GamConfAggArgs a) {
  __shared__ int bad;
  const int tid = threadIdx.x, b = blockIdx.x;
  int T = a.enc_len[b];
  T = T < 0 ? 0 : (T > a.Tp ? a.Tp : T);
  const int U = a.counts[b];
  const bool ulen_ok = U >= 0 && U <= a.cap;
  const int* y = a.ids + (size_t)b * a.cap;
  const int* fr = a.frames + (size_t)b * a.cap;
  if (tid == 0) bad = 0;
  __syncthreads();
  if (ulen_ok) {
    int e = 0;
    for (int u = tid; u < U; u += 256) {
      const int v = y[u], f = fr[u], prev = u > 0 ? fr[u - 1] : -1;
      e |= (v < 0 || v > a.V - 2 || f < 0 || f >= T || f <= prev);
    }
    if (e) atomicOr(&bad, 1);
  }
  __syncthreads();
  const bool valid = ulen_ok && bad == 0;
  if (tid == 0) a.status[b] = valid ? 1 : 0;
  float* cf = a.conf + (size_t)b * a.cap;
  int* sp = a.span + (size_t)b * a.cap;
  const int2* st = a.stats + (size_t)b * a.Tp;
  for (int u = tid; u < a.cap; u += 256) {
    if (!valid || u >= U) {
      cf[u] = -1.f;
      sp[u] = 0;
      continue;
    }
    int n;
    cf[u] = gam_ctc_conf_span(a.lp + (size_t)b * a.Tp * a.V, st, a.V, a.measure, a.agg, y[u], fr[u], u + 1 < U ? fr[u + 1] : T, n);
    sp[u] = n;
  }
}

// ------------------------------------------------------------------ CTC, ONE utterance of any length (gam_op_ctc_confidence_long)
// The contract above on one row with T in place of enc_len[b], plus the wildcard id V (`wildcard` = 1): a valid entry whose frame takes
// part in the increasing check and bounds its predecessor's span, itself not scored (conf -1, span 0).  Validity spans the whole grid,
// so it has a launch of its own: the stream zeroes ctrl[0], gam_ctc_conf_long_check_kernel ORs it and writes the clamped T to ctrl[1]
// (the enc_len word of gam_ctc_conf_stats_kernel, run with B = 1 and Tp = T), gam_ctc_conf_long_agg_kernel reads ctrl[0] and walks one
// span per thread with gam_ctc_conf_span: the batch op's statements, hence its bits on any stream the batch op takes.
struct GamConfLongArgs {
  const float* lp;         // [T, V]
  const int2* stats;       // [T]
  int* ctrl;               // [0] the list is invalid, [1] T (behind the stats in the handle's workspace)
  const int* ids;          // [cap]
  const int* frames;       // [cap]
  const int* count;        // [1]
  int T, V, cap, measure, agg, wildcard;
  float* conf;             // [cap]
  int* span;               // [cap]
  int* status;             // [1]
};

__global__ __launch_bounds__(256) void gam_ctc_conf_long_check_kernel(GamConfLongArgs a) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  const int U = a.count[0];
  const bool ulen_ok = U >= 0 && U <= a.cap;
  if (u == 0) {
    a.ctrl[1] = a.T;
    if (!ulen_ok) atomicOr(&a.ctrl[0], 1);
  }
  if (ulen_ok && u < U) {
    const int v = a.ids[u], f = a.frames[u], prev = u > 0 ? a.frames[u - 1] : -1;
    const bool id_ok = (v >= 0 && v <= a.V - 2) || (a.wildcard && v == a.V);
    if (!id_ok || f < 0 || f >= a.T || f <= prev) atomicOr(&a.ctrl[0], 1);
  }
}

__global__ __launch_bounds__(256) void gam_ctc_conf_long_agg_kernel(GamConfLongArgs a) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  const bool valid = a.ctrl[0] == 0;      // (valid: 0 <= U <= cap, every id and frame in range)
  if (u == 0) a.status[0] = valid ? 1 : 0;
  if (u >= a.cap) return;
  const int U = a.count[0];
  const int id = valid && u < U ? a.ids[u] : a.V;
  if (id == a.V) {                        // past the list, an invalid list, or a wildcard
    a.conf[u] = -1.f;
    a.span[u] = 0;
    return;
  }
  int n;
  a.conf[u] = gam_ctc_conf_span(a.lp, a.stats, a.V, a.measure, a.agg, id, a.frames[u], u + 1 < U ? a.frames[u + 1] : a.T, n);
  a.span[u] = n;
}

// ------------------------------------------------------------------ RNN-T 1: rows checked, outputs preset
struct GamRnntConfPrepArgs {
  const int* enc_len;      // [B]
  const int* ids;          // [B, cap]
  const int* frames;       // [B, cap]
  const int* counts;       // [B]
  int Tp, V, cap;
  float* conf;             // [B, cap] <- -1
  int* status;             // [B]
};

__global__ __launch_bounds__(256) void gam_rnnt_conf_prep_kernel(GamRnntConfPrepArgs a) {
  __shared__ int bad;
  const int tid = threadIdx.x, b = blockIdx.x;
  int T = a.enc_len[b];
  T = T < 0 ? 0 : (T > a.Tp ? a.Tp : T);
  const int U = a.counts[b];
  const bool ulen_ok = U >= 0 && U <= a.cap;
  if (tid == 0) bad = 0;
  __syncthreads();
  if (ulen_ok) {
    const int* y = a.ids + (size_t)b * a.cap;
    const int* fr = a.frames + (size_t)b * a.cap;
    int e = 0;
    for (int u = tid; u < U; u += 256) {
      const int v = y[u], f = fr[u], prev = u > 0 ? fr[u - 1] : 0;
      e |= (v < 0 || v > a.V - 2 || f < 0 || f >= T || f < prev);
    }
    if (e) atomicOr(&bad, 1);
  }
  __syncthreads();
  if (tid == 0) a.status[b] = ulen_ok && bad == 0 ? 1 : 0;
  for (int u = tid; u < a.cap; u += 256) a.conf[(size_t)b * a.cap + u] = -1.f;
}

// ------------------------------------------------------------------ RNN-T 2: the joint at the listed nodes
struct GamRnntConfArgs {
  const float* encp;       // [B, Tp, JH]
  const float* predp;      // [B, cap + 1, JH]: pp(y[:u]) at row u (gam_rnnt_tf_predict_kernel + the pp GEMM)
  const int* ids;          // [B, cap]
  const int* frames;       // [B, cap]
  const int* counts;       // [B]
  const int* status;       // [B] of gam_rnnt_conf_prep_kernel: rows of status 0 are not touched (their entries decide no address)
  const float* wout;       // [V, JH]
  const float* bout;       // [V]
  float* conf;             // [B, cap]
  int Tp, cap, V, JH, measure;
  float inv_lnv;
};

static inline size_t gam_cf_nodes_lds_bytes(int JH) { return sizeof(float) * 16 * (size_t)(JH + 4); }

__global__ __launch_bounds__(64) void gam_rnnt_conf_nodes_kernel(GamRnntConfArgs a) {
  extern __shared__ __attribute__((aligned(16))) float gam_smem_cf[];   // z [16][JH + 4]
  const int JH = a.JH, V = a.V, LD = JH + 4;
  const int lane = threadIdx.x, li = lane & 15, lg4 = lane >> 4;
  const int b = blockIdx.y, u0 = blockIdx.x * 16;
  if (a.status[b] == 0) return;
  const int U = a.counts[b];         // (status 1: 0 <= U <= cap, every id and frame in range)
  if (u0 >= U) return;
  const int* y = a.ids + (size_t)b * a.cap;
  const int* fr = a.frames + (size_t)b * a.cap;
  // z = relu(encp[frames[u]] + pp[u]) of the 16 tokens u0 .. u0 + 15 (clamped into the utterance: a clamped row is computed, not stored)
  const int q4 = JH >> 2;
  for (int e = lane; e < 16 * q4; e += 64) {
    const int r = e / q4, k = (e - r * q4) * 4;
    const int u = u0 + r < U ? u0 + r : U - 1;
    const f32x4 ef = gam_rc_glb4(a.encp + ((size_t)b * a.Tp + fr[u]) * JH + k);
    const f32x4 pf = gam_rc_glb4(a.predp + ((size_t)b * (a.cap + 1) + u) * JH + k);
    f32x4 z;
    z.x = fmaxf(ef.x + pf.x, 0.f); z.y = fmaxf(ef.y + pf.y, 0.f); z.z = fmaxf(ef.z + pf.z, 0.f); z.w = fmaxf(ef.w + pf.w, 0.f);
    *reinterpret_cast<f32x4*>(gam_smem_cf + (size_t)r * LD + k) = z;
  }
  __syncthreads();
  // C/D layout: column = lane & 15 = class, row = 4 (lane >> 4) + r = token u0 + 4 lg4 + r
  int yv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int u = u0 + 4 * lg4 + r;
    yv[r] = y[u < U ? u : U - 1];
  }
  float m[4], s[4], ax[4], xt[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY; s[r] = 0.f; ax[r] = 0.f; xt[r] = -INFINITY;
  }
  const float* zl = gam_smem_cf + li * LD + 4 * lg4;
  for (int nt0 = 0; nt0 * 16 < V; nt0 += GAM_CF_NV) {
    const float* wr[GAM_CF_NV];
    f32x4 acc[GAM_CF_NV], wf[GAM_CF_NV];
#pragma unroll
    for (int j = 0; j < GAM_CF_NV; ++j) {
      const int v = (nt0 + j) * 16 + li;
      wr[j] = a.wout + (size_t)(v < V ? v : V - 1) * JH + 4 * lg4;
      acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      wf[j] = gam_rc_glb4(wr[j]);
    }
    for (int k0 = 0; k0 < JH; k0 += 16) {
      const int kn = k0 + 16 < JH ? k0 + 16 : k0;       // the next k-step's W_out under this one's MFMAs
      f32x4 wn[GAM_CF_NV];
#pragma unroll
      for (int j = 0; j < GAM_CF_NV; ++j) wn[j] = gam_rc_glb4(wr[j] + kn);
      const f32x4 zf = gam_rc_lds4(zl + k0);
#pragma unroll
      for (int j = 0; j < GAM_CF_NV; ++j) {
        acc[j] = gam_mfma4(acc[j], zf, wf[j]);
      }
#pragma unroll
      for (int j = 0; j < GAM_CF_NV; ++j) wf[j] = wn[j];
    }
#pragma unroll
    for (int j = 0; j < GAM_CF_NV; ++j) {
      const int v = (nt0 + j) * 16 + li;
      if (v < V) {
        const float bo = a.bout[v];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float x = acc[j][r] + bo;
          const float nm = fmaxf(m[r], x);
          const float sc = gam_fast_exp(m[r] - nm), e = gam_fast_exp(x - nm);
          s[r] = s[r] * sc + e;
          ax[r] = ax[r] * sc + e * x;
          m[r] = nm;
          if (v == yv[r]) xt[r] = x;
        }
      }
    }
  }
  // the 16 lanes of a row hold the classes = li (mod 16): combine them, then lane 0 of the row stores its four tokens
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float M = gam_conf_row_max(m[r]);
    const float sc = m[r] > -INFINITY ? gam_fast_exp(m[r] - M) : 0.f;
    const float S = gam_conf_row_sum(s[r] * sc);
    const float A = gam_conf_row_sum(ax[r] * sc);
    const float X = gam_conf_row_max(xt[r]);
    const float lns = gam_fast_log(S);
    const int u = u0 + 4 * lg4 + r;
    if (li == 0 && u < U) {
      const float c = a.measure == GAM_CF_ENTROPY ? 1.0f - (M + lns - A / S) * a.inv_lnv : gam_fast_exp(X - M - lns);
      a.conf[(size_t)b * a.cap + u] = gam_conf_clamp01(c);
    }
  }
}
