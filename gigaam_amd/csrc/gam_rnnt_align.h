// gam_rnnt_align.h -- transducer forced alignment and transcript log-likelihood (gam_rnnt_align / gam_op_rnnt_align /
// gam_op_rnnt_lattice_align).
//
// The contract (shared with tests/rnnt_align_ref.py, float64).  The standard transducer lattice, the one the RNN-T loss sums over.
// For utterance b: T = enc_len[b], target y[0..U), blank = V - 1, nodes (t, u) with 0 <= t < T and 0 <= u <= U.
//   lb[t, u] = log P(blank | frame t, y[:u])            moves to (t + 1, u)
//   le[t, u] = log P(y[u] | frame t, y[:u]), u < U      moves to (t, u + 1)
//   with log P = log_softmax(W_out relu(encp[t] + pp(y[:u])) + b_out), pp(y) = W_pred g(y) + b_pred and g(y) the predictor's
//   output after feeding y from the zero state (the empty y: predict(None, None), gate_tab row V) -- gam_rnnt_beam.h's lp(t, y).
//   alpha[0, 0] = 0;  alpha[t, u] = logsumexp(alpha[t-1, u] + lb[t-1, u], alpha[t, u-1] + le[t, u-1])
//   log_likelihood = alpha[T-1, U] + lb[T-1, U]  (= -rnnt_loss);  score = the same with max instead of logsumexp (Viterbi)
//   tok_frame[u] = the frame t at which y[u] is emitted on the best path (the edge (t, u) -> (t, u + 1)): the meaning the greedy
//   decode's and the beam search's `frames` have.
// max_symbols_per_step does NOT bound the lattice: it is the loss's definition, not the decode's cap.  A best path may emit more
// than that many tokens in one frame, and the likelihood includes such paths.
// Tie rule (deterministic, shared with the reference): of two equal predecessors the blank predecessor (t-1, u) wins over the
// emission predecessor (t, u-1).
// Status 1: aligned (T = 0 with U = 0 included: score = loglik = 0).  Status 0: T = 0 with U > 0, a target id outside [0, V-2],
// target_len outside [0, Umax], or no path of finite score -- score = loglik = -inf, token frames -1.  Every T >= 1 is feasible
// for every U.  Token frames past target_len[b] are -1; target entries past target_len[b] are never read.
// Limits (host errors beyond them): Umax <= 1024, T' <= 8192, V <= 1025, pred_hidden and joint_hidden <= 512 (multiples of 16: every head
// gam_create accepts; the pp GEMM's K = pred_hidden runs with a zero-filled last k-tile when it is no multiple of 32, gam_gemm.h).
//
// Three kernels, exact fp32 products like the rest of the RNN-T head (MFMA f32 / fmaf chains, no fp16 terms):
//  1. gam_rnnt_tf_predict_kernel -- the teacher-forced predictor g[b, u], u = 0..U: ONE launch, one workgroup per utterance, u the
//     sequential loop.  The inputs are known in advance, and their input-side term W_ih embed(y[u-1]) + b_ih + b_hh is row y[u-1]
//     of the [V + 1, 4H] table gam_finalize builds for the decode kernels (a GEMM done once per model instead of once per call),
//     so the step is W_hh h alone (the greedy kernel's matvec).  pp = W_pred g + b_pred is then one GEMM over all (b, u).
//  2. gam_rnnt_lattice_kernel -- the fused joint.  A workgroup takes 32 frames x 16 target positions of one utterance; its wave w
//     takes 8 of those frames.  encp rows and pp rows sit in LDS; z = relu(encp[t] + pp[u]) is formed in registers as the MFMA's A
//     operand (16 target positions x 4 k per instruction, v_mfma_f32_16x16x4_f32), W_out is the B operand, read from L2 ONCE per
//     wave for its 128 nodes (prefetched one k-step ahead), the V tiles are reduced with an online log-sum-exp per lane and a
//     16-lane butterfly at the end, and only (lb, le) is stored: float2 [B, T', Umax + 1].  The logits never reach memory.
//  3. gam_rnnt_lattice_dp_kernel -- one workgroup per utterance sweeps the anti-diagonals d = t + u with ONE barrier per step;
//     thread u owns column u: its blank predecessor is its own value of the step before (a register), its emission predecessor
//     comes from thread u - 1 through LDS (double-buffered).  Viterbi max and forward log-sum-exp in the same sweep; every step
//     subtracts the previous diagonal's maximum (of each separately) into an fp64 offset: gam_trellis.h's frame.  Backpointers: 1 bit
//     per node as one 64-bit ballot per (diagonal, 64 columns); in LDS while (T' + Umax) x ceil((Umax + 1) / 64) x 8 B fit beside
//     the rest (BP_LDS), else in a global scratch buffer the handle owns.  The lattice values of diagonal d + GAM_RA_PF are loaded
//     while diagonal d is computed.  The backtrack runs in the same kernel (the thread that owns column U walks the bits).
// Workspace limit: the lattice of a call is B x T' x (Umax + 1) x 8 bytes.  When that exceeds the handle's limit
// (gam_set_rnnt_align_workspace, default 1 GiB) the host path processes the batch in slices of utterances, each slice's lattice
// within the limit (kernels 2 and 3 per slice, same results); one utterance that alone exceeds the limit is an error that names
// the bytes.
#pragma once
#include "gam_search.h"
#include "gam_decode.h"
#include "gam_trellis.h"

#define GAM_RA_MAX_U 1024
#define GAM_RA_MAX_T 8192
#define GAM_RA_MAX_H 512
#define GAM_RA_MAX_NT 1024
#define GAM_RA_MAX_SPT 2
#define GAM_RA_PF 4             // lattice diagonals in flight ahead of the step that uses them
#define GAM_RA_TF 32            // frames of one lattice workgroup (8 per wave)
#define GAM_RA_RT 8
#define GAM_RA_LDS_MAX (160 * 1024)
#define GAM_RA_WS_DEFAULT ((size_t)1 << 30)

// ------------------------------------------------------------------ 1. teacher-forced predictor
struct GamRnntTfArgs {
  const int* targets;      // [B, Umax]
  const int* target_len;   // [B]
  const float* gate_tab;   // [V+1, 4H]
  const float* whh_t;      // [H, 4H]
  const float* wih_x;      // [L-1][H][4H]
  const float* whh_x;      // [L-1][H][4H]
  const float* bias_x;     // [L-1][4H]
  float* g;                // [B, Umax+1, H]: the predictor output after y[:u]; rows u > U are zero
  int Umax, V, H, L;
};

static inline size_t gam_ra_tf_lds_bytes(int H, int L) { return sizeof(float) * ((size_t)L * 2 * H + 4 * H); }

template <int NR>   // gate rows per thread: 4 H <= 256 NR
__global__ __launch_bounds__(256) void gam_rnnt_tf_predict_kernel(GamRnntTfArgs a) {
  extern __shared__ __attribute__((aligned(16))) float gam_smem_ratf[];
  const int H = a.H, L = a.L, V = a.V, G = 4 * H;
  float* st = gam_smem_ratf;             // layer l: [h | c] at st + l * 2H
  float* gates = st + (size_t)L * 2 * H; // [4H]
  const int tid = threadIdx.x, b = blockIdx.x;
  int U = a.target_len[b];
  if (U < 0 || U > a.Umax) U = 0;        // (status 0 in the lattice sweep)
  const int* y = a.targets + (size_t)b * a.Umax;
  float* gb = a.g + (size_t)b * (a.Umax + 1) * H;
  for (int i = tid; i < L * 2 * H; i += 256) st[i] = 0.f;
  int roff[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) roff[j] = tid + 256 * j < G ? tid + 256 * j : G - 1;
  __syncthreads();
  for (int u = 0; u <= U; ++u) {
    int label = u == 0 ? V : y[u - 1];
    if (label < 0 || label > V - 2) label = V;   // (a bad id: status 0 in the lattice sweep; never an out-of-range row)
    for (int l = 0; l < L; ++l) {
      float* hs = st + (size_t)l * 2 * H;
      float acc[NR];
#pragma unroll
      for (int j = 0; j < NR; ++j)
        acc[j] = l == 0 ? a.gate_tab[(size_t)label * G + roff[j]] : a.bias_x[(size_t)(l - 1) * G + roff[j]];
      // acc[row] += sum_k Wt[k][row] vec[k]: 16 k x NR rows in flight, every load unconditional.  gam_decode.h's gam_rnnt_layer_step holds the
      // same step; this kernel keeps its own text because it measured 1.4 % slower on the shared one
      auto matvec = [&](const float* __restrict__ wt, const float* vec) {
        for (int k0 = 0; k0 < H; k0 += 16) {
          float w[16][NR];
#pragma unroll
          for (int kk = 0; kk < 16; ++kk)
#pragma unroll
            for (int j = 0; j < NR; ++j) w[kk][j] = wt[(size_t)(k0 + kk) * G + roff[j]];
#pragma unroll
          for (int kk = 0; kk < 16; ++kk) {
            const float hk = vec[k0 + kk];
#pragma unroll
            for (int j = 0; j < NR; ++j) acc[j] = fmaf(w[kk][j], hk, acc[j]);
          }
        }
      };
      if (l > 0) matvec(a.wih_x + (size_t)(l - 1) * H * G, hs - 2 * H);   // the NEW hidden state of the layer below
      matvec(l == 0 ? a.whh_t : a.whh_x + (size_t)(l - 1) * H * G, hs);
#pragma unroll
      for (int j = 0; j < NR; ++j)
        if (tid + 256 * j < G) gates[tid + 256 * j] = acc[j];
      __syncthreads();
      for (int i = tid; i < H; i += 256) {
        float c2, h2;
        gam_lstm_cell<false>(gates[i], gates[H + i], gates[2 * H + i], gates[3 * H + i], hs[H + i], c2, h2);
        hs[H + i] = c2;
        hs[i] = h2;
        if (l == L - 1) gb[(size_t)u * H + i] = h2;
      }
      __syncthreads();
    }
  }
  for (int i = (U + 1) * H + tid; i < (a.Umax + 1) * H; i += 256) gb[i] = 0.f;
}

// ------------------------------------------------------------------ 2. fused joint -> (lb, le)
struct GamRnntLatArgs {
  const float* encp;       // [B, Tp, JH]
  const float* predp;      // [B, Umax+1, JH]
  const int* enc_len;      // [B]
  const int* targets;      // [B, Umax]
  const int* target_len;   // [B]
  const float* wout;       // [V, JH]
  const float* bout;       // [V]
  float2* lat;             // [B, Tp, Umax+1] (lb, le); nodes t >= T or u > U are not written
  int Tp, Umax, V, JH;
};

static inline size_t gam_ra_lat_lds_bytes(int JH) { return sizeof(float) * (size_t)(16 + GAM_RA_TF) * (JH + 4); }

__global__ __launch_bounds__(256) void gam_rnnt_lattice_kernel(GamRnntLatArgs a) {
  extern __shared__ __attribute__((aligned(16))) float gam_smem_ralat[];
  const int JH = a.JH, V = a.V, LD = JH + 4, U1 = a.Umax + 1;
  float* pr = gam_smem_ralat;             // [16][LD] pp rows u0 .. u0 + 15
  float* en = pr + 16 * LD;               // [32][LD] encp rows t0 .. t0 + 31
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg4 = lane >> 4;
  const int b = blockIdx.z, u0 = blockIdx.y * 16, t0 = blockIdx.x * GAM_RA_TF;
  int T = a.enc_len[b];
  T = T < 0 ? 0 : (T > a.Tp ? a.Tp : T);
  const int U = a.target_len[b];
  if (U < 0 || U > a.Umax || t0 >= T || u0 > U) return;     // (block-uniform)
  // rows clamped into the utterance: a clamped row is computed and not stored
  const int q4 = JH >> 2;
  for (int e = tid; e < (16 + GAM_RA_TF) * q4; e += 256) {
    const int r = e / q4, k = (e - r * q4) * 4;
    const float* src;
    if (r < 16) {
      const int u = u0 + r < U1 ? u0 + r : U1 - 1;
      src = a.predp + ((size_t)b * U1 + u) * JH + k;
    } else {
      const int t = t0 + r - 16 < T ? t0 + r - 16 : T - 1;
      src = a.encp + ((size_t)b * a.Tp + t) * JH + k;
    }
    *reinterpret_cast<f32x4*>(gam_smem_ralat + (size_t)r * LD + k) = gam_rc_glb4(src);
  }
  __syncthreads();
  const int tw = t0 + GAM_RA_RT * wave;    // this wave's frames tw .. tw + 7
  if (tw >= T) return;
  // this lane's four target positions u0 + 4 lg4 + r: the id whose logit is le (-1: none)
  const int* y = a.targets + (size_t)b * a.Umax;
  int yv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int u = u0 + 4 * lg4 + r;
    int v = u < U ? y[u] : -1;
    yv[r] = (v < 0 || v > V - 2) ? -1 : v;
  }
  float m[GAM_RA_RT][4], s[GAM_RA_RT][4], xb[GAM_RA_RT][4], xe[GAM_RA_RT][4];
#pragma unroll
  for (int rt = 0; rt < GAM_RA_RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m[rt][r] = -INFINITY; s[rt][r] = 0.f; xb[rt][r] = -INFINITY; xe[rt][r] = -INFINITY;
    }
  const float* prl = pr + li * LD + 4 * lg4;
  const float* enl = en + (GAM_RA_RT * wave) * LD + 4 * lg4;
  for (int nt = 0; nt * 16 < V; ++nt) {
    const int v = nt * 16 + li;
    const float* wr = a.wout + (size_t)(v < V ? v : V - 1) * JH + 4 * lg4;
    f32x4 acc[GAM_RA_RT];
#pragma unroll
    for (int rt = 0; rt < GAM_RA_RT; ++rt) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 wf = gam_rc_glb4(wr);
    for (int k0 = 0; k0 < JH; k0 += 16) {
      const f32x4 wn = gam_rc_glb4(wr + (k0 + 16 < JH ? k0 + 16 : k0));   // the next k-step's W_out under this one's MFMAs
      const f32x4 pf = gam_rc_lds4(prl + k0);
#pragma unroll
      for (int rt = 0; rt < GAM_RA_RT; ++rt) {
        const f32x4 ef = gam_rc_lds4(enl + rt * LD + k0);
        const float z0 = fmaxf(ef.x + pf.x, 0.f), z1 = fmaxf(ef.y + pf.y, 0.f);
        const float z2 = fmaxf(ef.z + pf.z, 0.f), z3 = fmaxf(ef.w + pf.w, 0.f);
        acc[rt] = gam_mfma4(acc[rt], z0, z1, z2, z3, wf);
      }
      wf = wn;
    }
    // C/D: column = lane & 15 = class v, row = 4 (lane >> 4) + r = target position; this lane's running log-sum-exp of its classes
    if (v < V) {
      const float bo = a.bout[v];
#pragma unroll
      for (int rt = 0; rt < GAM_RA_RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float x = acc[rt][r] + bo;
          const float nm = fmaxf(m[rt][r], x);
          s[rt][r] = s[rt][r] * gam_fast_exp(m[rt][r] - nm) + gam_fast_exp(x - nm);
          m[rt][r] = nm;
          if (v == V - 1) xb[rt][r] = x;
          if (v == yv[r]) xe[rt][r] = x;
        }
    }
  }
  // the 16 lanes of a row group hold the classes = li (mod 16): butterfly to the full log-sum-exp, then the lanes that hold the
  // blank's and the target's logits store lb and le
  float* latf = reinterpret_cast<float*>(a.lat);
#pragma unroll
  for (int rt = 0; rt < GAM_RA_RT; ++rt) {
    const int t = tw + rt;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float M = m[rt][r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
      float S = m[rt][r] > -INFINITY ? s[rt][r] * gam_fast_exp(m[rt][r] - M) : 0.f;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) S += __shfl_xor(S, o, 64);
      const float lse = M + gam_fast_log(S);
      const int u = u0 + 4 * lg4 + r;
      if (t < T && u <= U) {
        const size_t o2 = (((size_t)b * a.Tp + t) * U1 + u) * 2;
        if (li == ((V - 1) & 15)) latf[o2] = xb[rt][r] - lse;
        if (yv[r] >= 0 ? li == (yv[r] & 15) : li == 0) latf[o2 + 1] = yv[r] >= 0 ? xe[rt][r] - lse : -INFINITY;
      }
    }
  }
}

// ------------------------------------------------------------------ 3. lattice sweep + backtrack
struct GamRnntDpArgs {
  const float2* lat;           // [B, Tp, Umax+1] (lb, le), read as they are (le at u = U is never used)
  const int* enc_len;          // [B]
  const int* targets;          // [B, Umax] or NULL (ids not checked)
  const int* target_len;       // [B]
  int Tp, Umax, V;
  int nchunk;                  // 64-column backpointer words per diagonal: ceil((Umax + 1) / 64)
  unsigned long long* bp_glob; // !BP_LDS: [B, Tp + Umax, nchunk]
  int* tok_frame;              // [B, Umax]
  float* score;                // [B]
  float* loglik;               // [B]
  int* status;                 // [B]
};

// LDS bytes of one workgroup (host and device carve it the same way)
static inline size_t gam_ra_dp_lds_bytes(bool bp_lds, int Tp, int Umax, int nchunk, int spt, int nt) {
  const size_t sp = ((size_t)spt * nt + 1 + 3) & ~(size_t)3;
  return (bp_lds ? (((size_t)(Tp + Umax) * nchunk * 8 + 15) & ~(size_t)15) : 0) + 16 * sp + GAM_TRELLIS_WM * sizeof(float) + 64;
}

template <bool BP_LDS, int SPT>   // SPT columns per thread: Umax + 1 <= SPT * blockDim
__global__ __launch_bounds__(GAM_RA_MAX_NT) void gam_rnnt_lattice_dp_kernel(GamRnntDpArgs a) {
  extern __shared__ uint4 gam_smem_radp[];
  unsigned char* smem = reinterpret_cast<unsigned char*>(gam_smem_radp);
  const int nt = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const int b = blockIdx.x;
  const int Tp = a.Tp, U1 = a.Umax + 1;
  const int sp = (SPT * nt + 1 + 3) & ~3;      // floats per buffer: a -inf sentinel (u - 1 of u = 0), then the columns
  unsigned long long* bpl = reinterpret_cast<unsigned long long*>(smem);
  float* XD = reinterpret_cast<float*>(smem + (BP_LDS ? (((size_t)(Tp + a.Umax) * a.nchunk * 8 + 15) & ~(size_t)15) : 0));   // XD[buf][1 + u]: node + le
  float* XA = XD + 2 * sp;
  float* wm = XA + 2 * sp;                       // per-wave maxima of the step (gam_trellis.h)
  int* misc = reinterpret_cast<int*>(wm + GAM_TRELLIS_WM);   // [1] bad id, [2] path found

  int T = a.enc_len[b];
  T = T < 0 ? 0 : (T > Tp ? Tp : T);
  const int U = a.target_len[b];
  const bool ulen_ok = U >= 0 && U <= a.Umax;
  if (tid < 4) misc[tid] = 0;
  __syncthreads();
  if (ulen_ok && a.targets != nullptr) {
    const int* y = a.targets + (size_t)b * a.Umax;
    int bad = 0;
    for (int u = tid; u < U; u += nt) {
      const int v = y[u];
      bad |= (v < 0 || v > a.V - 2);
    }
    if (bad) atomicOr(&misc[1], 1);
  }
  __syncthreads();
  int* tf = a.tok_frame + (size_t)b * a.Umax;
  const bool feasible = ulen_ok && misc[1] == 0 && (T >= 1 || U == 0);
  if (!feasible || T == 0) {      // (T == 0 and feasible: U == 0, the empty path)
    for (int u = tid; u < a.Umax; u += nt) tf[u] = -1;
    if (tid == 0) {
      a.score[b] = feasible ? 0.f : -INFINITY;
      a.loglik[b] = feasible ? 0.f : -INFINITY;
      a.status[b] = feasible ? 1 : 0;
    }
    return;
  }
  for (int k = tid; k < 2 * sp; k += nt) {
    XD[k] = -INFINITY;
    XA[k] = -INFINITY;
  }
  gam_trellis_wm_init(wm, tid);
  __syncthreads();

  // Lattice loads are unconditional (indices clamped into the utterance): a load under a branch would serialise the prefetch
  const float2* latb = a.lat + (size_t)b * Tp * U1;
  int uc[SPT];
  bool col[SPT];
  float bD[SPT], bA[SPT];     // node + lb of this thread's column at the step before
#pragma unroll
  for (int i = 0; i < SPT; ++i) {
    const int u = i * nt + tid;
    col[i] = u <= U;
    uc[i] = u <= U ? u : U;
    bD[i] = bA[i] = -INFINITY;
  }
  auto node = [&](int d, int i) {
    int t = d - (i * nt + tid);
    t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);
    return latb[(size_t)t * U1 + uc[i]];
  };
  float2 e[GAM_RA_PF][SPT];
#pragma unroll
  for (int k = 0; k < GAM_RA_PF; ++k)
#pragma unroll
    for (int i = 0; i < SPT; ++i) e[k][i] = node(k, i);

  const int ndiag = T + U;
  double offD = 0.0, offA = 0.0;   // what the renormalisations subtracted so far
  for (int d0 = 0; d0 < ndiag; d0 += GAM_RA_PF) {
#pragma unroll
    for (int k = 0; k < GAM_RA_PF; ++k) {
      const int d = d0 + k;
      if (d >= ndiag) break;
      const int cur = d & 1, prv = cur ^ 1;
      const float* XDp = XD + prv * sp;
      const float* XAp = XA + prv * sp;
      float* XDc = XD + cur * sp + 1;
      float* XAc = XA + cur * sp + 1;
      float mD, mA;
      gam_trellis_wm_read(wm, prv, mD, mA);
      offD += (double)mD;
      offA += (double)mA;
      float lmD = -INFINITY, lmA = -INFINITY;
      bool bpv[SPT];
#pragma unroll
      for (int i = 0; i < SPT; ++i) {
        const int u = i * nt + tid;
        const int t = d - u;
        bool bp = false;
        {
          float nd = -INFINITY, na = -INFINITY;
          if (col[i] && t >= 0 && t < T) {
            if (d == 0) {
              nd = 0.f;
              na = 0.f;
            } else {
              const float pb = bD[i], pe = XDp[u];       // blank predecessor (t-1, u), emission predecessor (t, u-1)
              bp = pe > pb;                              // a tie goes to the blank predecessor
              nd = (bp ? pe : pb) - mD;
              const float a0 = bA[i], a1 = XAp[u];
              const float M = fmaxf(a0, a1);
              if (M > -INFINITY) na = (M - mA) + gam_fast_log(gam_fast_exp(a0 - M) + gam_fast_exp(a1 - M));
            }
            lmD = fmaxf(lmD, nd);
            lmA = fmaxf(lmA, na);
          }
          const float lb = e[k][i].x, le = u < U ? e[k][i].y : -INFINITY;
          bD[i] = nd + lb;
          bA[i] = na + lb;
          XDc[u] = nd + le;
          XAc[u] = na + le;
        }
        bpv[i] = bp;
      }
      // the diagonal d + PF replaces the one just used (its load is in flight during the next PF - 1 steps)
#pragma unroll
      for (int i = 0; i < SPT; ++i) e[k][i] = node(d + GAM_RA_PF, i);
      gam_trellis_wm_publish(wm, cur, lane, wave, lmD, lmA);
#pragma unroll
      for (int i = 0; i < SPT; ++i) {
        const unsigned long long mk = __ballot(bpv[i]);
        const int c = i * nw + wave;
        if (lane == 0 && c < a.nchunk) {
          if (BP_LDS) bpl[(size_t)d * a.nchunk + c] = mk;
          else a.bp_glob[((size_t)b * (Tp + a.Umax) + d) * a.nchunk + c] = mk;
        }
      }
      __syncthreads();
    }
  }

  // the thread that owns column U holds (T-1, U) + lb[T-1, U] of the last diagonal: the results, then the walk back
  const int iU = U / nt;
  if (tid == U - iU * nt) {
    const float fD = iU == 0 ? bD[0] : bD[SPT - 1], fA = iU == 0 ? bA[0] : bA[SPT - 1];
    const bool found = fD > -INFINITY;
    a.score[b] = found ? (float)((double)fD + offD) : -INFINITY;
    a.loglik[b] = found && fA > -INFINITY ? (float)((double)fA + offA) : -INFINITY;
    a.status[b] = found ? 1 : 0;
    misc[2] = found ? 1 : 0;
    if (found) {
      int t = T - 1, u = U;
      while (u > 0) {
        const size_t w = (size_t)(t + u) * a.nchunk + (u >> 6);
        const unsigned long long mk = BP_LDS ? bpl[w] : a.bp_glob[(size_t)b * (Tp + a.Umax) * a.nchunk + w];
        if (((mk >> (u & 63)) & 1ull) || t == 0) {
          tf[u - 1] = t;
          --u;
        } else {
          --t;
        }
      }
    }
  }
  __syncthreads();
  for (int u = (misc[2] ? U : 0) + tid; u < a.Umax; u += nt) tf[u] = -1;
}
