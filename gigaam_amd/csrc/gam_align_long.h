// gam_align_long.h -- CTC forced alignment of ONE long utterance (gam_op_ctc_align_long), tiled over states and frames.
//
// The recurrences and the statuses are those of gam_align.h; the frame step, the tie rule, the backpointer encoding, the end rule and
// the feasibility rule are the same code, gam_trellis.h (read its header first).  What differs is the shape.  gam_align.h keeps
// the whole state row of an utterance in one workgroup's LDS (S <= 2049, T' <= 8192).
// Here the S = 2U + 1 states are cut into nS blocks of SB states (a multiple of 64) and the T frames into nT tiles of TT frames.
// Tile (j, k) = block j over time tile k needs
//   (a) block j's own state row at the end of tile k - 1, and
//   (b) the LAST state of block j - 1 at every frame t0 - 1 .. t1 - 2 of the tile [t0, t1).
// (SB is even, so a block starts on a blank state: its state 0 takes s - 1, its state 1 -- a token -- takes s - 2, both the
// neighbour's last state; the neighbour's state SB - 2 is never read from outside, so ONE edge state is published, not two.)
// Tile (j, k) runs in launch d = j + k: launch d holds one workgroup for every existing (j, k) on that anti-diagonal, (a) was written
// by launch d - 1 and (b) by launches d - 1 and d - 2.  STREAM ORDER IS THE ONLY DEPENDENCY: nT + nS - 1 plain launches, no flag, no
// spin, no grid sync, no graph -- no workgroup ever waits for a value a running workgroup produces.
//
// Precision: per block the scheme of gam_trellis.h -- each step subtracts the block's previous-step maximum (of d and of a), the
// offsets are carried in fp64 -- with the block's offsets and its last row kept in the workspace between tiles.  A block publishes
// its edge state per frame in ABSOLUTE terms as fp64 {d, a}; the reader subtracts its own fp64 offset and rounds to fp32 (one
// extra rounding of an O(frame log-prob) number per block edge and frame; -inf stays -inf).  A block whose states are all
// unreachable keeps offset 0 (the -inf -> 0 rule of gam_trellis.h).
//
// Backpointers: gam_trellis.h's chunk words, in a global workspace of T x ceil(S / 64) x 16 bytes.
// The whole workspace (backpointers + edges nS x T x 16 B + rows nS x SB x 8 B + path T x 4 B) is the handle's and is capped by
// gam_set_ctc_align_workspace / GAM_CTC_ALIGN_WS; the default cap GAM_AL_WS_DEFAULT = 3 GiB holds a one-hour recording with a
// char-level transcript (T = 9e4, U = 5e4: 2.25 GB of backpointers + 0.14 GB of edges).
//
// After the last sweep launch, on the same stream and with nothing going to the host: gam_ctc_align_long_backtrack (one wave: final
// score / loglik / status from the last block(s), then the pointer walk, 64 frames per step -- the path drops at most 2 states per
// frame, so 64 frames touch at most 3 chunks, which the wave fetches in one go and walks from LDS) writes path[T]; then
// gam_ctc_align_long_outputs (parallel over t) writes frame_labels / tok_first / tok_last, and every output of an infeasible call.
// Scores leave the device as float64.  Limits: T < 2^31, U whatever the workspace cap allows (state indices are 32-bit ints: the host
// entry point refuses U >= 2^30, far beyond what any cap that fits a GPU admits).
#pragma once
#include "gam_trellis.h"

#define GAM_AL_SB_DEFAULT 1024   // states per block: one state per thread of a 1024-thread workgroup
#define GAM_AL_TT_DEFAULT 256    // frames per tile
#define GAM_AL_SB_MAX (GAM_ALIGN_MAX_SPT * GAM_ALIGN_MAX_NT)
#define GAM_AL_WS_DEFAULT ((size_t)3 << 30)
// SB EVEN is load-bearing: only then does every block open on a blank state, which is why ONE published edge state per block is enough
// (see the header).  gam_tune_ctc_align_long admits multiples of 64 only; a rule relaxed to odd sizes would need the second edge state.
static_assert(GAM_AL_SB_DEFAULT % 64 == 0 && GAM_AL_SB_DEFAULT <= GAM_AL_SB_MAX, "blocks are whole 64-state chunks (and so even)");

struct GamAlignLongArgs {
  const float* lp;           // [T, V]
  const int* targets;        // [U]
  int T, V, U;
  int sb, tt, nS, nT;        // tiling: states per block, frames per tile, blocks, tiles
  int nchunk;                // 64-state backpointer chunks per frame: ceil(S / 64)
  int* ctrl;                 // {adjacent repeats, a bad id seen, a finite path found, -}; zeroed before the first kernel
  uint4* bp;                 // [T, nchunk] chunks of {bit0 lo, bit0 hi, bit1 lo, bit1 hi}
  float* rowD;               // [nS, sb] a block's d row at the end of its last tile, relative to off[j].x
  float* rowA;               // [nS, sb] the same for a, relative to off[j].y
  double2* off;              // [nS] what the block's renormalisations subtracted so far {of d, of a}
  double2* edge;             // [nS, T] absolute {d, a} of the block's last state (local SB - 1) per frame
  int* path;                 // [T] state per frame
  int* frame_labels;         // [T]
  int* tok_first;            // [U]
  int* tok_last;             // [U]
  double* score;
  double* loglik;
  int* status;
  static constexpr bool kStar = false;
};
// the STAR variant's arguments (target id V is the wildcard, gam_trellis.h): the old kernels keep their kernarg layout
struct GamAlignLongStarArgs : GamAlignLongArgs {
  const float* star;         // [T] the emission of a wildcard state per frame, read as it is
  static constexpr bool kStar = true;
};

// threads and states per thread of a block's workgroup: SB <= spt * nt, spt <= 3, nt a multiple of 64 up to 1024
static inline void gam_align_long_shape(int sb, int* nt, int* spt) {
  const int m = sb / 64;
  *spt = (m + 15) / 16;
  *nt = 64 * ((m + *spt - 1) / *spt);
}
static inline size_t gam_align_long_lds_bytes(int spt, int nt) { return 16 * ((size_t)spt * nt + 2) + GAM_TRELLIS_WM * sizeof(float); }
// tuning hook (gam_tune_ctc_align_long): 0 = the defaults above.  Process-wide like gam_tune_sp; the fields are atomics.
struct GamAlignLongForce { std::atomic<int> sb{0}, tt{0}; };
static inline GamAlignLongForce& gam_align_long_force() { static GamAlignLongForce f; return f; }

__device__ __forceinline__ bool gam_align_long_feasible(const GamAlignLongArgs& a) {
  return gam_ctc_feasible(a.T, a.U, a.ctrl[0], a.ctrl[1]);
}

// repeats and bad ids of the target (U > 0); STAR: id V is the wildcard
template <bool STAR = false>
__global__ __launch_bounds__(256) void gam_ctc_align_long_prep_kernel(GamAlignLongArgs a) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  int rep = 0, bad = 0;
  if (u < a.U) {
    const int v = a.targets[u];
    bad = gam_ctc_bad_id<STAR>(v, a.V);
    rep = u > 0 && a.targets[u - 1] == v;
  }
  const unsigned long long mr = __ballot(rep), mb = __ballot(bad);
  if ((threadIdx.x & 63) == 0) {
    if (mr) atomicAdd(&a.ctrl[0], __popcll(mr));
    if (mb) atomicOr(&a.ctrl[1], 1);
  }
}

// launch d of the sweep: workgroup x is tile (j, k) = (jlo + x, d - j), jlo = max(0, d - (nT - 1))
// Args = GamAlignLongStarArgs: the STAR variant, launched only by gam_op_ctc_align_long_star.
template <int SPT, typename Args = GamAlignLongArgs>
__global__ __launch_bounds__(GAM_ALIGN_MAX_NT) void gam_ctc_align_long_sweep_kernel(Args a, int d) {
  constexpr bool STAR = Args::kStar;
  extern __shared__ uint4 gam_smem_align_long[];
  if (!gam_align_long_feasible(a)) return;       // (before any emission load: a bad id would index outside lp)
  const int nt = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const int j = (d > a.nT - 1 ? d - (a.nT - 1) : 0) + blockIdx.x, k = d - j;
  const int T = a.T, V = a.V, blank = V - 1, sb = a.sb, S = 2 * a.U + 1;
  const int t0 = k * a.tt, t1 = a.tt < T - t0 ? t0 + a.tt : T;
  const int sp = SPT * nt + 2;                   // floats per state buffer: the neighbour's edge at [1] ([0] unused), then the states
  float* D = reinterpret_cast<float*>(gam_smem_align_long);   // D[buf][2 + local state], buf = t & 1
  float* A = D + 2 * sp;
  float* wm = A + 2 * sp;                        // per-wave maxima of the step (gam_trellis.h)

  // this thread's states: label, whether the s-2 skip is allowed
  int lab[SPT];
  bool act[SPT], skip[SPT];
  gam_ctc_lanes<SPT>(a.targets, blank, S, j * sb, sb, nt, tid, lab, act, skip);
  for (int q = tid; q < 2 * sp; q += nt) {
    D[q] = -INFINITY;
    A[q] = -INFINITY;
  }
  gam_trellis_wm_init(wm, tid);
  __syncthreads();

  // the row this tile starts from, in buffer prv of its first step: t = -1 is a virtual start that only state 0 holds
  const int pb = (t0 & 1) ^ 1;
  double offD = 0.0, offA = 0.0;                 // what the renormalisations subtracted so far
  // Block 0 has no neighbour: it loads its OWN edge row, which its own threads are writing meanwhile, so what it reads may be stale or
  // never written -- every use below is behind `j > 0 ?`, the value is discarded (this keeps a branch from round the load, gam_align.h).
  const double2* eg = a.edge + (size_t)(j > 0 ? j - 1 : 0) * T;
  if (k == 0) {
    if (j == 0 && tid == 0) {
      D[pb * sp + 2] = 0.f;
      A[pb * sp + 2] = 0.f;
    }
  } else {
    const double2 o = a.off[j];
    offD = o.x;
    offA = o.y;
    float lmD = -INFINITY, lmA = -INFINITY;
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
      const int sl = i * nt + tid;
      if (sl < sb) {
        const float vd = a.rowD[(size_t)j * sb + sl], va = a.rowA[(size_t)j * sb + sl];
        D[pb * sp + 2 + sl] = vd;
        A[pb * sp + 2 + sl] = va;
        lmD = fmaxf(lmD, vd);
        lmA = fmaxf(lmA, va);
      }
    }
    gam_trellis_wm_publish(wm, pb, lane, wave, lmD, lmA);
    if (tid == 0 && j > 0) {                     // the neighbour's last state at t0 - 1, in this block's frame of reference
      const double2 e = eg[t0 - 1];
      D[pb * sp + 1] = (float)(e.x - offD);
      A[pb * sp + 1] = (float)(e.y - offA);
    }
  }
  __syncthreads();

  // Emission and edge loads are unconditional (a row index clamped to t1 - 1, inactive states read the blank column): see gam_align.h
  // STAR: one unconditional load per state from the state's own (base, stride) -- gam_ctc_star_src
  const int ie = (sb - 1) / nt, te = (sb - 1) % nt;   // who holds local state SB - 1
  const float* src[SPT];
  int stride[SPT];
  if constexpr (STAR) gam_ctc_star_src<SPT>(a.lp, a.star, V, lab, src, stride);
  float e[GAM_ALIGN_PF][SPT];
  double2 ne[GAM_ALIGN_PF];
#pragma unroll
  for (int q = 0; q < GAM_ALIGN_PF; ++q) {
    const int tq = t0 + q < t1 ? t0 + q : t1 - 1;
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
      if constexpr (STAR) e[q][i] = src[i][(size_t)tq * stride[i]];
      else e[q][i] = a.lp[(size_t)tq * V + lab[i]];
    }
    ne[q] = eg[tq];
  }

  for (int tb = t0; tb < t1; tb += GAM_ALIGN_PF) {
#pragma unroll
    for (int q = 0; q < GAM_ALIGN_PF; ++q) {
      const int t = tb + q;
      if (t >= t1) break;
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
        bpv[i] = gam_ctc_step(Dp, Ap, Dc, Ac, i * nt + tid, act[i], skip[i], e[q][i], mD, mA, lmD, lmA, nd, na);
        if (i == ie && tid == te) a.edge[(size_t)j * T + t] = make_double2((double)nd + offD, (double)na + offA);
      }
      // the neighbour's last state at t, for the step t + 1, relative to this block's offsets after this step
      if (tid == 0) {
        Dc[-1] = j > 0 ? (float)(ne[q].x - offD) : -INFINITY;
        Ac[-1] = j > 0 ? (float)(ne[q].y - offA) : -INFINITY;
      }
      // the row t + PF replaces the one just used (its load is in flight during the next PF - 1 steps)
      const int tn = t + GAM_ALIGN_PF < t1 ? t + GAM_ALIGN_PF : t1 - 1;
#pragma unroll
      for (int i = 0; i < SPT; ++i) {
        if constexpr (STAR) e[q][i] = src[i][(size_t)tn * stride[i]];
        else e[q][i] = a.lp[(size_t)tn * V + lab[i]];
      }
      ne[q] = eg[tn];
      gam_trellis_wm_publish(wm, cur, lane, wave, lmD, lmA);
#pragma unroll
      for (int i = 0; i < SPT; ++i) {
        const int cl = i * nw + wave, c = j * (sb >> 6) + cl;
        gam_ctc_bp_pack(bpv[i], lane == 0 && cl < (sb >> 6) && c < a.nchunk, a.bp + ((size_t)t * a.nchunk + c));
      }
      __syncthreads();
    }
  }

  // what the next tile of this block (and, after the last tile, the backtrack kernel) starts from
  const int fb = (t1 - 1) & 1;
#pragma unroll
  for (int i = 0; i < SPT; ++i) {
    const int sl = i * nt + tid;
    if (sl < sb) {
      a.rowD[(size_t)j * sb + sl] = D[fb * sp + 2 + sl];
      a.rowA[(size_t)j * sb + sl] = A[fb * sp + 2 + sl];
    }
  }
  if (tid == 0) a.off[j] = make_double2(offD, offA);
}

// One wave behind the last sweep launch (T > 0): score / loglik / status from the last block(s), then the walk.
__global__ __launch_bounds__(64) void gam_ctc_align_long_backtrack_kernel(GamAlignLongArgs a) {
  __shared__ uint4 bpl[64 * 3];
  __shared__ int start[2];
  if (!gam_align_long_feasible(a)) return;       // (the outputs kernel writes every output of an infeasible call)
  const int lane = threadIdx.x, T = a.T, sb = a.sb, S = 2 * a.U + 1;
  if (lane == 0) {
    // states S - 1 and S - 2 at the last frame, absolute: S - 2 is the previous block's edge when S - 1 opens a block
    const int jl = (S - 1) / sb, l1 = (S - 1) % sb;
    const double2 o = a.off[jl];
    const double d1 = (double)a.rowD[(size_t)jl * sb + l1] + o.x, a1 = (double)a.rowA[(size_t)jl * sb + l1] + o.y;
    double d2 = -INFINITY, a2 = -INFINITY;
    if (S >= 2) {
      if (l1 > 0) {
        d2 = (double)a.rowD[(size_t)jl * sb + l1 - 1] + o.x;
        a2 = (double)a.rowA[(size_t)jl * sb + l1 - 1] + o.y;
      } else {
        const double2 e = a.edge[(size_t)(jl - 1) * T + T - 1];
        d2 = e.x;
        a2 = e.y;
      }
    }
    int s;
    double best, ll;
    const bool found = gam_ctc_end<double>(S, d1, d2, a1, a2, s, best, ll);
    *a.score = found ? best : -INFINITY;
    *a.loglik = ll;
    *a.status = found ? 1 : 0;
    a.ctrl[2] = found ? 1 : 0;
    start[0] = s;
    start[1] = found ? 1 : 0;
  }
  __syncthreads();
  if (!start[1]) return;
  int s = start[0];                              // (uniform: every lane walks the same path)
  for (int tb = T - 1; tb >= 0; tb -= 64) {
    // frames tb, tb - 1, .. (one per lane) x the chunk of s and the two below it: all the pointers these 64 steps can read
    const int c0 = s >> 6, t = tb - lane;
    if (t >= 1) {
#pragma unroll
      for (int q = 0; q < 3; ++q) bpl[lane * 3 + q] = a.bp[(size_t)t * a.nchunk + (c0 - q > 0 ? c0 - q : 0)];
    }
    __syncthreads();
    int mine = 0;
    const int n = tb + 1 < 64 ? tb + 1 : 64;
    for (int i = 0; i < n; ++i) {
      if (lane == i) mine = s;
      if (tb - i == 0) break;
      const uint4 w = bpl[i * 3 + (c0 - (s >> 6))];
      s -= gam_ctc_bp_step(w, s);
    }
    if (lane < n) a.path[t] = mine;
    __syncthreads();
  }
}

// frame labels and token runs from the path; every output of an infeasible call, of T = 0 and of a call that found no finite path
__global__ __launch_bounds__(256) void gam_ctc_align_long_outputs_kernel(GamAlignLongArgs a) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int T = a.T, U = a.U;
  const bool feasible = gam_align_long_feasible(a);
  if (!feasible || T == 0 || a.ctrl[2] == 0) {
    if (idx < T) a.frame_labels[idx] = -1;
    if (idx < U) a.tok_first[idx] = a.tok_last[idx] = -1;
    if (idx == 0 && (!feasible || T == 0)) {     // (T == 0 and feasible: U == 0, the empty path)
      *a.score = feasible ? 0.0 : -INFINITY;
      *a.loglik = feasible ? 0.0 : -INFINITY;
      *a.status = feasible ? 1 : 0;
    }
    return;
  }
  if (idx >= T) return;
  a.frame_labels[idx] = gam_ctc_frame_out(a.path, (int)idx, T, a.targets, a.V - 1, a.tok_first, a.tok_last);
}
