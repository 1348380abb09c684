// gam_align.h -- CTC forced alignment and transcript log-likelihood (gam_ctc_align / gam_op_ctc_align).
//
// For utterance b with log-probs lp[t, v] (t < T = enc_len[b], torch.log_softmax units), target y[0..U) and blank = V-1, the
// extended label sequence l = (blank, y0, blank, y1, ..., blank) has S = 2U + 1 states.  ONE sweep over t computes both
//   Viterbi  d_t(s) = lp[t, l_s] + max(d_{t-1}(s), d_{t-1}(s-1), d_{t-1}(s-2) if l_s != blank and l_s != l_{s-2})
//   forward  a_t(s) = the same recursion with log-sum-exp instead of max
// with score = max(d_{T-1}(S-1), d_{T-1}(S-2)) and log-likelihood = logsumexp(a_{T-1}(S-1), a_{T-1}(S-2)) (= -ctc_loss).
//
// Shape: one workgroup per utterance, states across the lanes (state s = i * blockDim + tid, i < SPT <= 3), t the sequential
// loop with ONE barrier per step (d / a double-buffered in LDS).  The emission row of frame t + GAM_ALIGN_PF is loaded while
// frame t is computed.  The frame step, its renormalisation (fp64 offsets), the tie rule, the backpointer encoding, the end rule
// and the feasibility rule are gam_trellis.h's, shared with gam_align_long.h.  Backpointers sit in LDS when T' x chunks x 16 B
// fit beside the rest of the workgroup's LDS (BP_LDS), else in a global scratch buffer the handle owns.  The backtrack runs in
// the same kernel (one lane walks the 2-bit pointers, then every lane writes).
//
// Limits: U <= GAM_ALIGN_MAX_U (S <= 2049) tokens, T' <= GAM_ALIGN_MAX_T frames (the host entry points fail beyond them).
// Infeasible utterances -- T < U + #{i : y_i == y_{i-1}}, a target id outside [0, V-2], target_len outside [0, Umax], or no
// path of finite score -- get status 0, score = loglik = -inf, frame labels and token frames -1; target entries past
// target_len[b] are never read.  U = 0 is the all-blank path; T = 0 with U = 0 scores 0.
//
// The STAR variant (gam_ctc_align_star / gam_op_ctc_align_star) admits target id V, the wildcard of gam_trellis.h, whose emission is
// star[b, t]; everything else, the statuses included, is as above with [0, V-2] + {V} for the ids.
#pragma once
#include "gam_trellis.h"

#define GAM_ALIGN_MAX_U 1024
#define GAM_ALIGN_MAX_T 8192
#define GAM_ALIGN_LDS_MAX (160 * 1024)

struct GamAlignArgs {
  const float* lp;           // [B, Tp, V]
  const int* enc_len;        // [B]
  const int* targets;        // [B, Umax] (may be NULL when Umax == 0)
  const int* target_len;     // [B]
  int Tp, V, Umax;
  int nchunk;                // 64-state backpointer chunks per frame: ceil(S_max / 64)
  uint4* bp_glob;            // !BP_LDS: [B, Tp, nchunk] chunks of {bit0 lo, bit0 hi, bit1 lo, bit1 hi}
  int* frame_labels;         // [B, Tp]
  int* tok_first;            // [B, Umax]
  int* tok_last;             // [B, Umax]
  float* score;              // [B]
  float* loglik;             // [B]
  int* status;               // [B]
  static constexpr bool kStar = false;
};
// the STAR variant's arguments: the old kernels keep their kernarg layout
struct GamAlignStarArgs : GamAlignArgs {
  const float* star;         // [B, Tp] the emission of a wildcard state (target id V) per frame, read as it is
  static constexpr bool kStar = true;
};

// LDS bytes of one workgroup (host and device carve it the same way)
static inline size_t gam_align_lds_bytes(bool bp_lds, int Tp, int nchunk, int spt, int nt) {
  const size_t sp = (size_t)spt * nt + 2;
  return (bp_lds ? (size_t)Tp * nchunk * 16 : 0) + 16 * sp + GAM_TRELLIS_WM * sizeof(float) + 64 + (((size_t)Tp * 2 + 15) & ~(size_t)15);
}

// Wildcard row: star[b, t] = max_v lp[b, t, v] - penalty for t < enc_len[b] (enc_len NULL: every row), 0 past it (never read).  One
// wave per row with coalesced reads, as gam_kws_rowmax_kernel -- a sibling, because that one leaves the rows past enc_len unwritten and
// writes {m, blank - m} pairs the keyword search reads as they are.
__global__ __launch_bounds__(256) void gam_ctc_star_row_kernel(const float* __restrict__ lp, const int* __restrict__ enc_len, int Tp, int V,
                                                               long rows, float penalty, float* __restrict__ star) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int b = (int)(row / Tp), t = (int)(row - (long)b * Tp);
  if (enc_len != nullptr && t >= enc_len[b]) {
    if (lane == 0) star[row] = 0.f;
    return;
  }
  const float* p = lp + (size_t)row * V;
  float m = -INFINITY;
  for (int v = lane; v < V; v += 64) m = fmaxf(m, p[v]);
  m = gam_wave_max(m);
  if (lane == 0) star[row] = m - penalty;
}

// Args = GamAlignStarArgs: the STAR variant (target id V is the wildcard, gam_trellis.h), launched only by the star entry points.
template <bool BP_LDS, int SPT, typename Args = GamAlignArgs>   // SPT states per thread: S_max <= SPT * blockDim
__global__ __launch_bounds__(GAM_ALIGN_MAX_NT) void gam_ctc_align_kernel(Args a) {
  constexpr bool STAR = Args::kStar;
  extern __shared__ uint4 gam_smem_align[];
  unsigned char* smem = reinterpret_cast<unsigned char*>(gam_smem_align);
  const int nt = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const int b = blockIdx.x;
  const int Tp = a.Tp, V = a.V, blank = V - 1;
  const int sp = SPT * nt + 2;                   // floats per state buffer: two -inf sentinels (s - 1, s - 2 of s = 0), then states
  size_t off = BP_LDS ? (size_t)Tp * a.nchunk * 16 : 0;
  uint4* bpl = gam_smem_align;
  float* D = reinterpret_cast<float*>(smem + off);     // D[buf][2 + s], buf = t & 1
  float* A = D + 2 * sp;
  float* wm = A + 2 * sp;                              // per-wave maxima of the step (gam_trellis.h)
  int* misc = reinterpret_cast<int*>(wm + GAM_TRELLIS_WM);   // repeats, bad id, path found
  // the six output pointers, parked in LDS across the sweep: held in SGPRs through it they made the kernel spill SGPRs
  void** outp = reinterpret_cast<void**>(misc + 4);
  unsigned short* path = reinterpret_cast<unsigned short*>(misc + 16);

  int T = a.enc_len[b];
  T = T < 0 ? 0 : (T > Tp ? Tp : T);
  const int U = a.target_len[b];
  const bool ulen_ok = U >= 0 && U <= a.Umax;
  const int* y = a.targets + (size_t)b * a.Umax;
  if (tid < 4) misc[tid] = 0;
  if (tid == 0) {
    outp[0] = a.frame_labels; outp[1] = a.tok_first; outp[2] = a.tok_last;
    outp[3] = a.score; outp[4] = a.loglik; outp[5] = a.status;
  }
  __syncthreads();
  if (ulen_ok) {
    int reps = 0, bad = 0;
    for (int u = tid; u < U; u += nt) {
      const int v = y[u];
      bad |= gam_ctc_bad_id<STAR>(v, V);
      reps += (u > 0 && y[u - 1] == v);
    }
    if (reps) atomicAdd(&misc[0], reps);
    if (bad) atomicOr(&misc[1], 1);
  }
  __syncthreads();
  const int S = 2 * U + 1;
  int* fl = a.frame_labels + (size_t)b * Tp;
  int* tf = a.tok_first + (size_t)b * a.Umax;
  int* tl = a.tok_last + (size_t)b * a.Umax;
  const bool feasible = ulen_ok && gam_ctc_feasible(T, U, misc[0], misc[1]);
  if (!feasible || T == 0) {      // (T == 0 and feasible: U == 0, the empty path)
    for (int t = tid; t < Tp; t += nt) fl[t] = -1;
    for (int u = tid; u < a.Umax; u += nt) tf[u] = tl[u] = -1;
    if (tid == 0) {
      a.score[b] = feasible ? 0.f : -INFINITY;
      a.loglik[b] = feasible ? 0.f : -INFINITY;
      a.status[b] = feasible ? 1 : 0;
    }
    return;
  }

  // this thread's states: label, whether the s-2 skip is allowed
  int lab[SPT];
  bool act[SPT], skip[SPT];
  gam_ctc_lanes<SPT>(y, blank, S, 0, S, nt, tid, lab, act, skip);
  // t = -1: a virtual start that only state 0 holds (then d_0(0) = lp[0, blank], d_0(1) = lp[0, y0], the rest -inf)
  for (int k = tid; k < 2 * sp; k += nt) {
    D[k] = -INFINITY;
    A[k] = -INFINITY;
  }
  gam_trellis_wm_init(wm, tid);
  __syncthreads();
  if (tid == 0) {
    D[sp + 2] = 0.f;
    A[sp + 2] = 0.f;
  }
  __syncthreads();

  // Emission loads are unconditional (a row index clamped to T - 1, inactive states read the blank column): a load under a branch makes
  // hipcc wait for every load in flight at its first use, which would serialise the prefetch.
  // STAR: the load stays ONE unconditional load per state, from the state's own (base, stride) -- gam_ctc_star_src.
  const float* lpb = a.lp + (size_t)b * Tp * V;
  const float* src[SPT];
  int stride[SPT];
  if constexpr (STAR) gam_ctc_star_src<SPT>(lpb, a.star + (size_t)b * Tp, V, lab, src, stride);
  float e[GAM_ALIGN_PF][SPT];
#pragma unroll
  for (int k = 0; k < GAM_ALIGN_PF; ++k)
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
      if constexpr (STAR) e[k][i] = src[i][(size_t)(k < T ? k : T - 1) * stride[i]];
      else e[k][i] = lpb[(size_t)(k < T ? k : T - 1) * V + lab[i]];
    }

  double offD = 0.0, offA = 0.0;   // what the renormalisations subtracted so far
  for (int t0 = 0; t0 < T; t0 += GAM_ALIGN_PF) {
#pragma unroll
    for (int k = 0; k < GAM_ALIGN_PF; ++k) {
      const int t = t0 + k;
      if (t >= T) break;
      const int cur = t & 1, prv = cur ^ 1;
      const float* Dp = D + prv * sp + 2;
      const float* Ap = A + prv * sp + 2;
      float* Dc = D + cur * sp + 2;
      float* Ac = A + cur * sp + 2;
      float mD, mA;
      gam_trellis_wm_read(wm, prv, mD, mA);
      offD += (double)mD;
      offA += (double)mA;
      float lmD = -INFINITY, lmA = -INFINITY;
      unsigned bpv[SPT];
#pragma unroll
      for (int i = 0; i < SPT; ++i) {
        float nd, na;
        bpv[i] = gam_ctc_step(Dp, Ap, Dc, Ac, i * nt + tid, act[i], skip[i], e[k][i], mD, mA, lmD, lmA, nd, na);
      }
      // the row t + PF replaces the one just used (its load is in flight during the next PF - 1 steps)
      const int tn = t + GAM_ALIGN_PF < T ? t + GAM_ALIGN_PF : T - 1;
#pragma unroll
      for (int i = 0; i < SPT; ++i) {
        if constexpr (STAR) e[k][i] = src[i][(size_t)tn * stride[i]];
        else e[k][i] = lpb[(size_t)tn * V + lab[i]];
      }
      gam_trellis_wm_publish(wm, cur, lane, wave, lmD, lmA);
#pragma unroll
      for (int i = 0; i < SPT; ++i) {
        const int c = i * nw + wave;
        if (BP_LDS) gam_ctc_bp_pack(bpv[i], lane == 0 && c < a.nchunk, bpl + ((size_t)t * a.nchunk + c));
        else gam_ctc_bp_pack(bpv[i], lane == 0 && c < a.nchunk, a.bp_glob + (((size_t)b * Tp + t) * a.nchunk + c));
      }
      __syncthreads();
    }
  }

  fl = reinterpret_cast<int*>(outp[0]) + (size_t)b * Tp;
  tf = reinterpret_cast<int*>(outp[1]) + (size_t)b * a.Umax;
  tl = reinterpret_cast<int*>(outp[2]) + (size_t)b * a.Umax;
  if (tid == 0) {
    float* score = reinterpret_cast<float*>(outp[3]);
    float* loglik = reinterpret_cast<float*>(outp[4]);
    int* status = reinterpret_cast<int*>(outp[5]);
    const int fb = (T - 1) & 1;
    const float* Df = D + fb * sp + 2;
    const float* Af = A + fb * sp + 2;
    int s;
    float best, ll;
    const bool found = gam_ctc_end<float>(S, Df[S - 1], S >= 2 ? Df[S - 2] : -INFINITY, Af[S - 1], S >= 2 ? Af[S - 2] : -INFINITY, s, best, ll);
    score[b] = found ? (float)((double)best + offD) : -INFINITY;
    loglik[b] = ll > -INFINITY ? (float)((double)ll + offA) : -INFINITY;
    status[b] = found ? 1 : 0;
    misc[2] = found ? 1 : 0;
    if (found) {
      for (int t = T - 1; t >= 0; --t) {
        path[t] = (unsigned short)s;
        if (t == 0) break;
        const uint4 w = BP_LDS ? bpl[(size_t)t * a.nchunk + (s >> 6)] : a.bp_glob[((size_t)b * Tp + t) * a.nchunk + (s >> 6)];
        s -= gam_ctc_bp_step(w, s);
      }
    }
  }
  __syncthreads();
  if (!misc[2]) {
    for (int t = tid; t < Tp; t += nt) fl[t] = -1;
    for (int u = tid; u < a.Umax; u += nt) tf[u] = tl[u] = -1;
    return;
  }
  for (int t = tid; t < Tp; t += nt) fl[t] = t < T ? gam_ctc_frame_out(path, t, T, y, blank, tf, tl) : -1;
  for (int u = U + tid; u < a.Umax; u += nt) tf[u] = tl[u] = -1;
}
