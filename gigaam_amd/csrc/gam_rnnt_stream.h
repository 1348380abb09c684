// gam_rnnt_stream.h -- gam_decode.h's one-workgroup RNN-T greedy decode for ONE stream of any length fed in pieces
// (gam_op_rnnt_greedy_stream).
//
// The frame / symbol loop is gam_rnnt_greedy_loop, the batch kernel's own: this kernel only says where frames come from (rows 0 .. n - 1
// of the call's encp are stream frames t_base .. t_base + n - 1), where tokens go (token k of the stream at ids[k] / frames[k], frames as
// stream frames) and where the state starts and ends (the record below).  Every (frame, state) is therefore evaluated with the batch
// kernel's arithmetic, and since a joint window's rows do not depend on each other, a stream cut anywhere -- inside a window too -- gives
// the bits of the uncut one.
//
// State record (caller-owned, gam_rnnt_greedy_stream_bytes): GamRnntStreamHdr | 2 L H floats, layer l's committed h at [2 l H], its
// committed c at [2 l H + H].  What is NOT stored, and why nothing is lost:
//   * the candidate (h', c') and W_pred g: a call recomputes them from the committed state and the last label before its first
//     window (need_pred = true at the loop's entry) -- the same inputs through the same code, hence the same bits;
//   * the symbols emitted on the current frame (`sym`): a call ends only when its last frame has ended, by a blank or at max_symbols,
//     so sym is 0 at every cut (gam_rnnt_greedy_loop; tests/test_rnnt_stream_host.py proves it on the float64 twin).
// A call: check the call against the record, load the state into LDS (BEGIN: zeros and the no-label row, predict(None, None)), run the
// loop over the n rows, store the state, the header, count[0] and status[0] = 1.  Nothing is stored to the record inside the loop.  All
// state and result stores are plain per-lane stores.  n = 0 is legal with either flag, both or none.
// Refusals (status[0] = 0, nothing else written, the record unchanged): without BEGIN, a record that was not begun or has ended, a
// t_base that is not the record's next frame, max_symbols / V / H / JH / L other than BEGIN recorded; with or without BEGIN,
// count + n * max_symbols > cap (the call could overflow ids / frames).
#pragma once
#include "gam_decode.h"

#define GAM_RNNT_F_BEGIN 1                // include/gigaam_hip.h GAM_RNNT_STREAM_BEGIN / _END
#define GAM_RNNT_F_END 2
#define GAM_RNNT_ST_MAGIC 0x726e7453      // anything else, zeros included, is "not begun"

struct GamRnntStreamHdr {
  int magic, begun, ended, count;         // count: tokens so far
  long long next;                         // the next stream frame
  int label;                              // the last token (V: none yet)
  int max_symbols, V, H, JH, L;
  int pad[4];
};
static_assert(sizeof(GamRnntStreamHdr) == 64 && offsetof(GamRnntStreamHdr, next) == 16, "RNN-T stream state layout");

static inline size_t gam_rnnt_stream_bytes(int H, int L) { return sizeof(GamRnntStreamHdr) + (size_t)2 * (L > 1 ? L : 1) * H * sizeof(float); }

struct GamRnntStreamArgs {
  GamRnntArgs a;         // the weights and sizes; encp [n, JH] of this call; ids / frames [cap] of the stream; no dump
  int n, t_base, flags;
  void* state;
  int* count;            // [1]
  int* status;           // [1]
};

template <int NR>   // gate rows per thread: 4*H <= 256*NR
__global__ __launch_bounds__(256) void gam_rnnt_greedy_stream_kernel(GamRnntStreamArgs g) {
  extern __shared__ __attribute__((aligned(16))) float gam_smem_rnnt_stream[];
  const GamRnntArgs& a = g.a;
  const int H = a.H, V = a.V;
  const int L = a.L > 1 ? a.L : 1;
  const int tid = threadIdx.x;
  GamRnntStreamHdr* hdr = static_cast<GamRnntStreamHdr*>(g.state);
  float* st = reinterpret_cast<float*>(hdr + 1);

  // ---- the call against the record (every thread reads the header before the first barrier; it is written behind the last)
  const bool begin = (g.flags & GAM_RNNT_F_BEGIN) != 0;
  int label = V, n_out = 0, n_dump = 0;
  bool ok = true;
  if (!begin) {
    ok = hdr->magic == GAM_RNNT_ST_MAGIC && hdr->begun == 1 && hdr->ended == 0 && hdr->next == (long long)g.t_base &&
         hdr->max_symbols == a.max_symbols && hdr->V == V && hdr->H == H && hdr->JH == a.JH && hdr->L == L && hdr->count >= 0 &&
         hdr->label >= 0 && hdr->label <= V;
    if (ok) { label = hdr->label; n_out = hdr->count; }
  }
  ok = ok && (long long)n_out + (long long)g.n * a.max_symbols <= (long long)a.cap;
  if (!ok) {
    if (tid == 0) g.status[0] = 0;
    return;
  }

  const GamRnntLds s = gam_rnnt_carve(gam_smem_rnnt_stream, H, a.JH, V, a.wout_in_lds);
  for (int i = tid; i < H; i += 256) { s.h_s[i] = begin ? 0.f : st[i]; s.c_s[i] = begin ? 0.f : st[H + i]; }
  for (int i = tid; i < (L - 1) * 2 * H; i += 256) {     // layer l1 + 1: [h | c] of the record -> [h | c | . | .] of xs
    const int l1 = i / (2 * H), r = i - l1 * 2 * H;
    s.xs[(size_t)l1 * 4 * H + r] = begin ? 0.f : st[(size_t)(l1 + 1) * 2 * H + r];
  }
  if (g.n > 0) gam_rnnt_load_wout(s, a.wout, V, a.JH, tid);
  __syncthreads();

  gam_rnnt_greedy_loop<NR>(a, s, a.encp, g.n, a.ids, a.frames, a.cap, g.t_base, nullptr, label, n_out, n_dump);

  // ---- store the state (the loop left the workgroup behind a barrier), then the header
  for (int i = tid; i < H; i += 256) { st[i] = s.h_s[i]; st[H + i] = s.c_s[i]; }
  for (int i = tid; i < (L - 1) * 2 * H; i += 256) {
    const int l1 = i / (2 * H), r = i - l1 * 2 * H;
    st[(size_t)(l1 + 1) * 2 * H + r] = s.xs[(size_t)l1 * 4 * H + r];
  }
  if (tid == 0) {
    hdr->magic = GAM_RNNT_ST_MAGIC;
    hdr->begun = 1;
    hdr->ended = (g.flags & GAM_RNNT_F_END) ? 1 : 0;
    hdr->count = n_out;
    hdr->next = (long long)g.t_base + g.n;
    hdr->label = label;
    hdr->max_symbols = a.max_symbols; hdr->V = V; hdr->H = H; hdr->JH = a.JH; hdr->L = L;
    g.count[0] = n_out;
    g.status[0] = 1;
  }
}
