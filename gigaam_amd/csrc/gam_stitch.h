// gam_stitch.h -- one long recording as ONE CTC utterance without a speech detector: the recording is cut into fixed overlapping
// windows that are encoded as a batch (gigaam_amd/windows.py plans them), and
//   gam_ctc_stitch_kernel        copies the kept frames of every window's log-probs into one [T_total, V] stream, bit for bit;
//   gam_ctc_greedy_long_*        CTCGreedyDecoding.decode (reference gigaam/decoding.py:56-96) of ONE utterance of any length, spread over
//                                the whole GPU -- gam_ctc_greedy_kernel keeps an utterance's labels in one workgroup's LDS, which an
//                                hour of audio (90 000 frames) does not fit.
// Both are plain launches in stream order; no workgroup ever waits for another one (no look-back, no cooperative launch, no device-wide
// barrier), nothing is atomic, and every store is a vector store.
#pragma once
#include "gam_common.h"

// ------------------------------------------------------------------ stitch
// Utterance b contributes rows lo[b] <= t < min(hi[b], enc_len[b]) of log_probs[b] to out[dst[b] + t - lo[b]].  The kept rows of one
// utterance are contiguous in the source AND in the destination, so the copy is one flat run of n x V floats: grid (chunks, B), every
// workgroup walks its utterance's run with a grid stride.  Access width: the widest of 16 / 8 / 4 bytes at which the source and the
// destination address are congruent (V = 34: rows are 8-byte aligned only, and lo / dst of different parity leave 8 bytes); up to W - 1
// floats in front of the first aligned destination address and behind the last whole vector are copied one by one.
//   status[b] = 1: nothing was clipped (0 <= lo, hi <= enc_len clamped to [0, T']) and the destination rows lie inside [0, T_total);
//   hi <= lo copies nothing and is no error (status 1).  A clipped window still copies its valid rows; a window whose destination rows
//   do not all fit copies NOTHING (status 0): no byte outside `out` is ever written.
struct GamStitchArgs {
  const float* lp;       // [B, Tp, V]
  const int* enc_len;    // [B]
  const int* lo;         // [B]
  const int* hi;         // [B]
  const long long* dst;  // [B]
  float* out;            // [T_total, V]
  int* status;           // [B]
  long long Tp, T_total;
  int V;
};

template <int W>
__device__ __forceinline__ void gam_stitch_run(const float* __restrict__ s, float* __restrict__ d, long long total, int bx, int nbx, int tid) {
  typedef float vecW __attribute__((ext_vector_type(W)));
  // floats in front of the first W-aligned destination address (the source is congruent: it is aligned there too)
  long long head = (long long)((W - (int)((reinterpret_cast<size_t>(d) >> 2) & (W - 1))) & (W - 1));
  head = head < total ? head : total;
  const long long nvec = (total - head) / W;
  const long long tail0 = head + nvec * W;
  const vecW* sv = reinterpret_cast<const vecW*>(s + head);
  vecW* dv = reinterpret_cast<vecW*>(d + head);
  for (long long i = (long long)bx * 256 + tid; i < nvec; i += (long long)nbx * 256) dv[i] = sv[i];
  if (bx == 0) {        // (head, tail < W <= 4)
    if (tid < head) d[tid] = s[tid];
    if (tail0 + tid < total && tid < W) d[tail0 + tid] = s[tail0 + tid];
  }
}
template <>
__device__ __forceinline__ void gam_stitch_run<1>(const float* __restrict__ s, float* __restrict__ d, long long total, int bx, int nbx, int tid) {
  for (long long i = (long long)bx * 256 + tid; i < total; i += (long long)nbx * 256) d[i] = s[i];
}

__global__ __launch_bounds__(256) void gam_ctc_stitch_kernel(GamStitchArgs a) {
  const int b = blockIdx.y, tid = threadIdx.x;
  int len = a.enc_len[b];
  len = len < 0 ? 0 : ((long long)len > a.Tp ? (int)a.Tp : len);
  const int lo = a.lo[b], hi = a.hi[b];
  const long long dst = a.dst[b];
  int ok = 1;
  long long n = 0, d0 = 0;
  int lo_c = lo;
  if (hi > lo) {
    lo_c = lo < 0 ? 0 : lo;
    const int hi_c = hi > len ? len : hi;
    if (lo < 0 || hi > len) ok = 0;                       // clipped: the valid rows are still copied
    n = hi_c > lo_c ? (long long)(hi_c - lo_c) : 0;
    d0 = dst + ((long long)lo_c - (long long)lo);          // out row of source row lo_c
    if (n > 0 && (d0 < 0 || d0 > a.T_total || n > a.T_total - d0)) { ok = 0; n = 0; }   // does not fit: nothing is written
  }
  if (blockIdx.x == 0 && tid == 0) a.status[b] = ok;
  if (n == 0) return;                                     // (block-uniform)
  const float* s = a.lp + ((size_t)b * (size_t)a.Tp + (size_t)lo_c) * (size_t)a.V;
  float* d = a.out + (size_t)d0 * (size_t)a.V;
  const long long total = n * (long long)a.V;
  const size_t diff = reinterpret_cast<size_t>(s) ^ reinterpret_cast<size_t>(d);   // equal low bits = congruent addresses
  if ((diff & 15) == 0) gam_stitch_run<4>(s, d, total, blockIdx.x, gridDim.x, tid);
  else if ((diff & 7) == 0) gam_stitch_run<2>(s, d, total, blockIdx.x, gridDim.x, tid);
  else gam_stitch_run<1>(s, d, total, blockIdx.x, gridDim.x, tid);
}

// ------------------------------------------------------------------ greedy decode of one long utterance
// Three launches in stream order over blocks of FB frames (GAM_GL_FB = 512 in the one-thread-per-frame form; GAM_GL_FBW = 128 in the
// one-wave-per-frame form, where a block of 512 frames would leave a third of the CUs without a workgroup at one hour of audio):
//   labels   per-frame argmax (torch's first-maximum tie rule; blank = V - 1) of the block's frames AND of the one frame before it,
//            which is recomputed instead of read from the neighbour's result; keep[t] = label[t] != blank && (t == 0 || label[t] !=
//            label[t - 1]).  Writes lab[t] = label (kept) or -1 - label (dropped) and the block's keep count.
//   scan     ONE workgroup turns the block counts into exclusive offsets, in place, and writes count = their sum (T = 0: 0).
//   compact  every block writes its kept (label, frame) pairs at its offset, in frame order (ballot / popcount prefix).
// The two argmax forms are those of gam_ctc_greedy_kernel (gam_decode.h): one thread per frame for even V <= 64, one wave per frame
// with gam_first_max otherwise.  Workspace: lab [T] | blk [ceil(T / FB)] ints, the handle's.
#define GAM_GL_FB 512      // threads per block of the labels kernel; frames per block in the one-thread-per-frame form
#define GAM_GL_FBW 128     // frames per block in the one-wave-per-frame form (8 waves x 16 rows)
#define GAM_GL_SCAN_NT 1024
#define GAM_GL_NL 16       // wave-per-frame form: loads of one lane in flight per row (16 x 64 classes = 1024 per pass) ...
#define GAM_GL_NR 4        // ... and rows of one wave in flight

template <int FB>   // frames per block
__global__ __launch_bounds__(GAM_GL_FB) void gam_ctc_greedy_long_labels_kernel(const float* __restrict__ lp, long long T, int V, int* __restrict__ lab_out,
                                                                               int* __restrict__ blk_count) {
  __shared__ int lab[FB + 1];                 // lab[j] = label of frame t0 - 1 + j
  __shared__ int wtot[GAM_GL_FB / 64];
  constexpr int NWV = GAM_GL_FB / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long t0 = (long long)blockIdx.x * FB;
  const int blank = V - 1;
  const long long nfr = T - t0 < FB ? T - t0 : FB;                  // frames of this block (>= 1)
  const int j0 = t0 == 0 ? 1 : 0;                                   // frame -1 does not exist
  if (FB == GAM_GL_FB) {       // (the launcher's choice: even V <= 64)
    const int hv = V >> 1;
    for (int j = tid; j <= (int)nfr; j += GAM_GL_FB) {
      if (j < j0) continue;
      const float2* xr = reinterpret_cast<const float2*>(lp + (size_t)(t0 - 1 + j) * V);   // (V even: 8-byte aligned rows)
      float2 x[32];
#pragma unroll
      for (int k = 0; k < 32; ++k) x[k] = xr[k < hv ? k : 0];
      float best = -INFINITY;
      int bi = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        if (k < hv) {    // ascending class order + strict '>' = first maximum
          if (x[k].x > best || bi == 0x7fffffff) { best = x[k].x; bi = 2 * k; }
          if (x[k].y > best) { best = x[k].y; bi = 2 * k + 1; }
        }
      }
      lab[j] = bi;
    }
  } else {
    // GAM_GL_NR rows of a wave and GAM_GL_NL loads per lane and row in flight before the first compare (a plain strided loop keeps ONE
    // load outstanding: 17 dependent L2 round trips per row at V = 1025; one row at a time leaves 4 KB per wave in flight).  Every load
    // is unconditional: the class index is clamped into the row, the row index into the block.
    for (int jb = j0 + wave; jb <= (int)nfr; jb += NWV * GAM_GL_NR) {
      float best[GAM_GL_NR];
      int bi[GAM_GL_NR];
      const float* xr[GAM_GL_NR];
#pragma unroll
      for (int r = 0; r < GAM_GL_NR; ++r) {
        const int jr = jb + NWV * r <= (int)nfr ? jb + NWV * r : (int)nfr;
        xr[r] = lp + (size_t)(t0 - 1 + jr) * V;
        best[r] = -INFINITY;
        bi[r] = 0x7fffffff;
      }
      for (int v0 = lane; v0 < V; v0 += 64 * GAM_GL_NL) {
        float x[GAM_GL_NR][GAM_GL_NL];
#pragma unroll
        for (int r = 0; r < GAM_GL_NR; ++r)
#pragma unroll
          for (int k = 0; k < GAM_GL_NL; ++k) x[r][k] = xr[r][v0 + 64 * k < V ? v0 + 64 * k : V - 1];
#pragma unroll
        for (int r = 0; r < GAM_GL_NR; ++r)
#pragma unroll
          for (int k = 0; k < GAM_GL_NL; ++k) {
            const int v = v0 + 64 * k;
            if (v < V && (x[r][k] > best[r] || (x[r][k] == best[r] && v < bi[r]))) { best[r] = x[r][k]; bi[r] = v; }
          }
      }
#pragma unroll
      for (int r = 0; r < GAM_GL_NR; ++r) {
        gam_first_max<64>(best[r], bi[r]);
        // (no comparable value in the row -- all NaN: class 0, as the thread form)
        if (lane == 0 && jb + NWV * r <= (int)nfr) lab[jb + NWV * r] = bi[r] == 0x7fffffff ? 0 : bi[r];
      }
    }
  }
  __syncthreads();
  bool keep = false;
  if (tid < nfr) {
    const int l = lab[tid + 1];
    keep = (l != blank) && (t0 + tid == 0 || l != lab[tid]);
    lab_out[t0 + tid] = keep ? l : -1 - l;
  }
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wtot[wave] = __popcll(m);
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
#pragma unroll
    for (int w = 0; w < NWV; ++w) tot += wtot[w];
    blk_count[blockIdx.x] = tot;
  }
}

// exclusive scan of blk[0 .. nblk) in place, count[0] = the total.  One workgroup: nblk = T / FB entries (176 / 704 for an hour of audio).
__global__ __launch_bounds__(GAM_GL_SCAN_NT) void gam_ctc_greedy_long_scan_kernel(int* __restrict__ blk, int nblk, int* __restrict__ count) {
  __shared__ int wtot[GAM_GL_SCAN_NT / 64];
  constexpr int NWV = GAM_GL_SCAN_NT / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (int base = 0; base < nblk; base += GAM_GL_SCAN_NT) {
    const int i = base + tid;
    const int v = i < nblk ? blk[i] : 0;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NWV; ++w) {
      const int c = wtot[w];
      woff += w < wave ? c : 0;
      tot += c;
    }
    if (i < nblk) blk[i] = carry + woff + incl - v;
    carry += tot;
    __syncthreads();
  }
  if (tid == 0) count[0] = carry;
}

template <int FB>   // frames per block = threads per block, as the labels kernel's
__global__ __launch_bounds__(FB) void gam_ctc_greedy_long_compact_kernel(const int* __restrict__ lab, const int* __restrict__ blk_off, long long T,
                                                                                int* __restrict__ ids, int* __restrict__ frames) {
  __shared__ int wtot[FB / 64];
  constexpr int NWV = FB / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long t = (long long)blockIdx.x * FB + tid;
  const int l = t < T ? lab[t] : -1;
  const bool keep = l >= 0;
  const unsigned long long m = __ballot(keep);
  const int before = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wtot[wave] = __popcll(m);
  __syncthreads();
  int woff = 0;
#pragma unroll
  for (int w = 0; w < NWV; ++w) woff += w < wave ? wtot[w] : 0;
  if (keep) {
    const long long pos = (long long)blk_off[blockIdx.x] + woff + before;   // < T: at most one kept pair per frame
    ids[pos] = l;
    frames[pos] = (int)t;
  }
}
