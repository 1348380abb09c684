// gam_rnnt_beam.h -- RNN-T beam search with hotword boosting (gam_rnnt_beam / gam_op_rnnt_beam).
//
// The contract (shared with tests/rnnt_beam_ref.py, which holds real token tuples).  For utterance b: T = enc_len[b], blank = V - 1,
// beam width W (1..32), K = min(W, V - 1) candidate tokens per joint row, S = max_symbols (1..16).  A hypothesis h has its token
// sequence y, the predictor state after feeding y (the empty y: predict(None, None), gate_tab row V, as in gam_rnnt_greedy_kernel),
// pp(y) = W_pred g(y) + b_pred, a score (log-prob) and a hotword state (node, acc, committed) with the rules of gam_search.h.
//   lp(t, y) = log_softmax(W_out relu(encp[t] + pp(y)) + b_out);   rank = score + committed + acc.
//
//   beam = {empty: score 0}
//   for t in 0 .. T-1:
//     B = {}; A_0 = beam
//     for s in 0 .. S:
//       if s < S: for a in A_s (position p): lp = lp(t, a.y)
//                   blank candidate  (a.y, a.score + lp[blank]), origin key (s, p, 0)          -> merged into B
//                   for v in the top-K non-blank ids of lp (ties to the lower id):
//                     extension (a.y + v, a.score + lp[v]), emitted at frame t, key (s, p, v + 1), hotword step -> C_s
//       else:     for a in A_S: (a.y, a.score), key (S, p, 0) -> merged into B    (forced advance without a joint: greedy's rule)
//       theta = the W-th highest rank in B, or -inf while |B| < W
//       A_{s+1} = top W of {c in C_s : rank(c) > theta}; the frame ends when it is empty
//       one predictor step for A_{s+1}'s new last tokens (all rows together), then W_pred
//     beam = top W of B
//   final: the entry of beam with the best score + committed (ties: lower position)
// Merging in B: entries with equal y are log-add-exp'd; the merged entry keeps the prefix node (its frames) and the predictor state of
// the contributor with the higher score (= higher rank: the hotword state depends on y alone), ties to the earlier (smaller key)
// contributor, and the key of its first contributor.  Within one C_s sequences are distinct.  Every top-W selection breaks rank ties
// by the smaller origin key.  The theta cut is part of the contract: without it C_s is never empty and every frame runs S joints and S
// predictor steps; with it a blank-dominant frame ends after one joint.
// Hypothesis identity: (length, 64-bit hash), gam_search.h.
//
// Shape: one workgroup of GAM_RB_NT threads per utterance; t the sequential loop; the backtrack at the end of the same kernel.
//   joint   z [rows][JH] = relu(encp[t] + pp) in LDS; logits = z W_out^T + b_out on the matrix cores (v_mfma_f32_16x16x4_f32, rows
//           padded to 16 or 32, W_out read from L2 ONCE per call for all rows) into a per-utterance global scratch slice; then one
//           wave per row: log-sum-exp, blank and the top K (64-bit keys, wave maxima: gam_beam_wave_topn).
//   merge   wave 0: blank / forced candidates into B (hash compare), theta, the top W extensions -> A_{s+1} (prefix-trie nodes,
//           predictor-state slots from a free list).
//   predict gates = gate_tab[v] + W_hh h (layer 0; layers above take the new h of the layer below through W_ih) for all rows at once,
//           four gate tiles of 16 hidden units per MFMA pass so the LSTM cell runs on the accumulators; then pp = W_pred g + b_pred.
//           The states live in global slots [L][h | c] | pp of a per-utterance pool of (S + 1) W slots: the beam holds <= W, each
//           A_{s+1} takes <= W fresh ones, and the free list is rebuilt from the new beam at the end of every frame.
// Arithmetic: exact fp32 (MFMA f32, expf / logf), no fp16 terms.  Every row's sums run in the same order whatever its position, so
// one y always gets bit-identical predictor outputs.  Renormalisation: each frame subtracts the best kept rank from the scores and adds
// it to an fp64 offset.  Limits (host errors beyond them): W <= 32, S <= 16, T' <= 8192, V <= 1025, H and JH <= 512 (multiples of 16).
//
// N-best (template <bool NBEST>; gam_rnnt_beam_nbest): the final pick becomes gam_search.h's emission of the n best entries of the
// final beam; everything before it is the same code.
//
// Word n-gram LM (template <bool LM>; gam_rnnt_beam_kernel<false> is the kernel without it, unchanged; tests/rnnt_beam_ref.py with an
// LMSpec is the float64 reference).  The word rules of gam_search.h, applied to hypotheses: token classes from gam_set_lm (0 continues the current
// word, 1 starts a new word, 2 separates; blank is class 0 and never extends y).  A hypothesis carries the spelling hash of its
// partial word (0 = empty), its last order - 1 completed word ids (<s> at the start) and lm, the LM term so far.
//   rank = score + committed + acc + lm.
//   An extension a.y + v with class(v) in {1, 2} whose a has a non-empty partial word completes that word: it adds
//   d(a) = alpha ln P(w | state) + beta and w enters the state; class 0 appends v to the partial word, class 1 starts the partial
//   word [v], class 2 leaves it empty.  Blank candidates and the forced advance at s = S leave the LM state as it is.
//   Equal y means equal LM state, so the merge in B is unchanged (it keeps the first contributor's state).  The theta cut and every
//   top-W selection use this rank.
//   Final pick: the last partial word is completed, then alpha ln P(</s> | state) is added: best score + committed + lm.
//   score = log p + committed + lm (final); logp is unchanged.  Renormalisation subtracts the best rank minus its lm.
//   With alpha = beta = 0 every lm and d is +0, so ids, frames, score and logp are bit-identical to the kernel without the LM.
// Cost: one LM query per NEW hypothesis, not per candidate: d(a) and w's id depend on a alone, so wave 0 queries them for every entry
// of A_{s+1} whose partial word is non-empty, right after its top-W selection, and the next joint phase only adds d to the
// extensions by class-1/2 tokens (the split of gam_search.h).  The LM state of the A lists and of B (36 B per entry) and the class
// table [V] i8 lie in LDS after the union region (gam_rb_lm_bytes): 22.4 KiB at W = 32, S = 16, V = 1025.
//
// One stream fed in pieces (template <bool STREAM>; gam_rnnt_beam_stream.h holds the contract of that form and its kernel): the same
// text with every difference behind `if constexpr (STREAM)` -- the beam comes from and goes to a caller-owned record, rows are stream
// frames, nodes are int4, score / logp are fp64.  The <.., false> instantiations compile what they compiled without it.
#pragma once
#include <type_traits>
#include "gam_search.h"

#define GAM_RB_NT 256
#define GAM_RB_MAX_S 16
#define GAM_RB_MAX_H 512
#define GAM_RB_MAX_T 8192

struct GamRnntBeamArgs {
  const float* encp;     // [B*Tp, JH]
  const int* enc_len;    // [B]
  const float* gate_tab; // [V+1, 4H]
  const float* whh_t;    // [H, 4H]
  const float* wpred_t;  // [H, JH]
  const float* bpred;    // [JH]
  const float* wout;     // [V, JH]
  const float* bout;     // [V]
  const float* wih_x;    // [L-1][H][4H]
  const float* whh_x;    // [L-1][H][4H]
  const float* bias_x;   // [L-1][4H]
  int Tp, V, H, JH, L, W, K, S;
  GamHwArgs hw;
  float* ws;             // [B][slots (S+1) W x SS | logits Wp x LGS] floats
  size_t ws_stride;      // floats per utterance
  int2* nodes;           // [B][Tp S W]
  int* ids;              // [B, cap]
  int* frames;           // [B, cap]
  int cap;
  int* counts;           // [B]
  float* score;          // [B]
  float* logp;           // [B]
  GamLmArgs lm;
  GamNbestArgs nb;       // the <.., true> kernels only: ids / frames are then [B, n, cap], counts / score / logp [B, n]
};
// (the kernel argument layout the fields had before the two blocks were structs of their own; the N-best block is appended)
static_assert(sizeof(GamRnntBeamArgs) == 304 && offsetof(GamRnntBeamArgs, hw) == 120 && offsetof(GamRnntBeamArgs, ws) == 144 &&
              offsetof(GamRnntBeamArgs, lm) == 216 && offsetof(GamRnntBeamArgs, nb) == 288, "GamRnntBeamArgs layout");

// LDS carve (host and device), in bytes, in this order: A lists [2][32] (hash u64; len, score, hotword node, acc, committed, prefix
// node, slot, token, parent slot: i32 / f32), row blank log-probs [32], counters [16], B list [P] (hash u64; len, score, best
// contributor score, key, slot, node, hotword node, acc, committed), free list [P], slot mask [(P + 31) / 32], then from a 16-byte
// boundary the union region U (joint rows z [Wp][JH + 4] | candidates [W K] (key u64; score, acc, committed, hotword node) | hidden
// rows [1 or 2][Wp][H + 4]), then with the LM (gam_rb_lm_bytes) the LM state of the A lists [2][32] and of the B list [P] (index
// buf * 32 + i and 64 + i: word state int4, partial-word hash u64, lm, d, completed word id) and the classes [V] i8, then the hotword
// trie when it lies in LDS.
__host__ __device__ static inline size_t gam_rb_pool(int W, int S) { return (size_t)(S + 1) * W; }
__host__ __device__ static inline size_t gam_rb_fixed_bytes(int W, int S) {
  const size_t P = gam_rb_pool(W, S);
  const size_t f = 2 * 32 * 8 + 2 * 32 * 9 * 4 + 32 * 4 + 16 * 4 + P * 8 + P * 9 * 4 + P * 4 + ((P + 31) / 32) * 4;
  return (f + 15) & ~(size_t)15;
}
__host__ __device__ static inline size_t gam_rb_union_bytes(int W, int K, int H, int JH, int L) {
  const size_t Wp = (size_t)((W + 15) / 16) * 16;
  size_t u = Wp * (JH + 4) * 4;
  const size_t c = (size_t)W * K * (8 + 4 * 4);
  const size_t hb = (size_t)(L > 1 ? 2 : 1) * Wp * (H + 4) * 4;
  u = u > c ? u : c;
  u = u > hb ? u : hb;
  return (u + 15) & ~(size_t)15;
}
__host__ __device__ static inline size_t gam_rb_lm_bytes(int W, int S, int V) {
  const size_t n = 64 + gam_rb_pool(W, S);
  return (n * (16 + 8 + 3 * 4) + (size_t)V + 15) & ~(size_t)15;
}
// lm_V: the class table's V with the LM, 0 without
static inline size_t gam_rb_lds_bytes(int W, int K, int S, int H, int JH, int L, int hw_lds_words, int lm_V = 0) {
  return gam_rb_fixed_bytes(W, S) + gam_rb_union_bytes(W, K, H, JH, L) + (lm_V > 0 ? gam_rb_lm_bytes(W, S, lm_V) : 0) +
         (size_t)hw_lds_words * 4;
}
// floats of one utterance's global workspace: the state slots and the logit rows
static inline size_t gam_rb_ws_floats(int W, int S, int V, int H, int JH, int L) {
  const size_t Wp = (size_t)((W + 15) / 16) * 16;
  return gam_rb_pool(W, S) * ((size_t)L * 2 * H + JH) + Wp * (size_t)((V + 3) & ~3);
}

// ---- the stream form (template <bool STREAM>; gam_rnnt_beam_stream.h holds its contract and its kernel): the record one stream's search
// is carried in from call to call, and what a call adds to GamRnntBeamArgs.  The batch instantiations read none of it.
#define GAM_RB_STREAM_REBASE 256          // a power of two
#define GAM_RB_F_BEGIN 1                  // include/gigaam_hip.h GAM_RNNT_STREAM_BEGIN / _END
#define GAM_RB_F_END 2
#define GAM_RB_ST_BEGUN 0x72626d73        // phase words; anything else, zeros included, is "not begun"
#define GAM_RB_ST_ENDED 0x72626d65

struct GamRbStreamHdr {
  int phase, W, S, V, H, JH, L;
  int hw_gen, lm_gen;
  int nb, ncount;                 // beam size, prefix-trie nodes so far
  int next, max_frames, t0;       // the next stream frame, the node pool's frames, the frame BEGIN started at
  int pad0[2];
  double off, cb_off, lm_off;     // what the renormalisations / the rebases of the committed bonus / of the LM term subtracted so far
  int pad1[10];
};
struct GamRbStreamEntry {         // one entry of A list 0; the LM fields are zeros without the LM, every field is zero beyond the beam
  unsigned long long h;
  int len;
  float sc;
  int hn;
  float acc, cb;
  int node, slot, pad0;
  unsigned long long wh;
  int4 ctx;
  float lm, dl;
  int cw, pad1;
};
static_assert(sizeof(GamRbStreamHdr) == 128 && offsetof(GamRbStreamHdr, off) == 64 && sizeof(GamRbStreamEntry) == 80 &&
              offsetof(GamRbStreamEntry, ctx) == 48, "RNN-T beam stream state layout");
#define GAM_RB_STREAM_HDR_BYTES (sizeof(GamRbStreamHdr) + 32 * sizeof(GamRbStreamEntry))      // 2688: the slot pool starts here

struct GamRbStreamArgs {
  int n, t_base, max_frames, flags;     // max_frames: what the caller's state_bytes hold for this W, S and head
  int hw_gen, lm_gen;
  void* state;
  int* status;           // [1]
  double* score;         // [1]   (END only, as ids / frames / counts[0] of GamRnntBeamArgs)
  double* logp;          // [1]
};

// acc[g][rt] += A[16 rt + i][k] * Wt[k][g * H + j0 + c] over k < H: A rows from LDS (row stride H + 4), Wt k-major with 4H columns.
// MFMA lane (i = lane & 15, q = lane >> 4): A row i, weight column j0 + i, k = k0 + 4 q + e in the e-th MFMA of a group of four.
template <int RT>
__device__ __forceinline__ void gam_rb_gates_mm(f32x4 (&acc)[4][2], const float* A, const float* __restrict__ Wt, int H, int j0, int li,
                                                int lg4) {
  const int G = 4 * H, ALD = H + 4;
  for (int k0 = 0; k0 < H; k0 += 16) {
    float w[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int g = 0; g < 4; ++g) w[g][e] = Wt[(size_t)(k0 + 4 * lg4 + e) * G + g * H + j0 + li];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const f32x4 a = gam_rc_lds4(A + (16 * rt + li) * ALD + k0 + 4 * lg4);
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g][rt] = gam_mfma4(acc[g][rt], a, w[g]);
    }
  }
}

// STREAM: a holds one utterance (encp [n, JH], ids / frames [cap], counts [1], ws = the logit rows alone); x the call and the record.
template <int RT, bool LM, bool NBEST, bool STREAM>
__device__ __forceinline__ void gam_rb_body(const GamRnntBeamArgs& a, const GamRbStreamArgs& x);

template <bool LM, bool NBEST = false>
__global__ __launch_bounds__(GAM_RB_NT) void gam_rnnt_beam_kernel(GamRnntBeamArgs a) {
  if (a.W > 16) gam_rb_body<2, LM, NBEST, false>(a, GamRbStreamArgs{});
  else gam_rb_body<1, LM, NBEST, false>(a, GamRbStreamArgs{});
}

template <int RT, bool LM, bool NBEST, bool STREAM>
__device__ __forceinline__ void gam_rb_body(const GamRnntBeamArgs& a, const GamRbStreamArgs& x) {
  static_assert(!(STREAM && NBEST), "there is no N-best over a stream");
  using Node = typename std::conditional<STREAM, int4, int2>::type;      // {parent, token, stream frame, 0} | {parent, token << 13 | frame}
  extern __shared__ uint4 gam_smem_rbeam[];
  unsigned char* p = reinterpret_cast<unsigned char*>(gam_smem_rbeam);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg4 = lane >> 4;
  const int b = blockIdx.x;
  const int Tp = a.Tp, V = a.V, H = a.H, JH = a.JH, L = a.L, W = a.W, K = a.K, S = a.S, blank = V - 1;
  const int Wp = 16 * RT, G = 4 * H;
  const int P = (S + 1) * W;
  const size_t SS = (size_t)L * 2 * H + JH;        // slot: [L][h | c] | pp
  const int LGS = (V + 3) & ~3;
  auto take = [&](size_t n) { unsigned char* r = p; p += n; return r; };
  unsigned long long* ah = reinterpret_cast<unsigned long long*>(take(2 * 32 * 8));   // A lists [buf * 32 + i]
  int* alen = reinterpret_cast<int*>(take(2 * 32 * 4));
  float* asc = reinterpret_cast<float*>(take(2 * 32 * 4));
  int* ahn = reinterpret_cast<int*>(take(2 * 32 * 4));
  float* aacc = reinterpret_cast<float*>(take(2 * 32 * 4));
  float* acb = reinterpret_cast<float*>(take(2 * 32 * 4));
  int* anode = reinterpret_cast<int*>(take(2 * 32 * 4));
  int* aslot = reinterpret_cast<int*>(take(2 * 32 * 4));
  int* atok = reinterpret_cast<int*>(take(2 * 32 * 4));
  int* apar = reinterpret_cast<int*>(take(2 * 32 * 4));
  float* rlpb = reinterpret_cast<float*>(take(32 * 4));
  int* cnt = reinterpret_cast<int*>(take(16 * 4));      // [0], [1]: sizes of the A lists
  unsigned long long* bh = reinterpret_cast<unsigned long long*>(take((size_t)P * 8));
  int* blen = reinterpret_cast<int*>(take((size_t)P * 4));
  float* bsc = reinterpret_cast<float*>(take((size_t)P * 4));
  float* bcs = reinterpret_cast<float*>(take((size_t)P * 4));
  int* bkey = reinterpret_cast<int*>(take((size_t)P * 4));
  int* bslot = reinterpret_cast<int*>(take((size_t)P * 4));
  int* bnode = reinterpret_cast<int*>(take((size_t)P * 4));
  int* bhn = reinterpret_cast<int*>(take((size_t)P * 4));
  float* bacc = reinterpret_cast<float*>(take((size_t)P * 4));
  float* bcb = reinterpret_cast<float*>(take((size_t)P * 4));
  int* freel = reinterpret_cast<int*>(take((size_t)P * 4));
  int* smask = reinterpret_cast<int*>(take((size_t)((P + 31) / 32) * 4));
  p = reinterpret_cast<unsigned char*>(gam_smem_rbeam) + gam_rb_fixed_bytes(W, S);
  unsigned char* U = p;
  // the union region: joint rows | candidates | hidden rows
  float* zr = reinterpret_cast<float*>(U);
  const int NC = W * K;
  unsigned long long* ckey = reinterpret_cast<unsigned long long*>(U);
  float* csc = reinterpret_cast<float*>(U + (size_t)NC * 8);
  float* cacc = csc + NC;
  float* ccb = cacc + NC;
  int* chn = reinterpret_cast<int*>(ccb + NC);
  float* hx = reinterpret_cast<float*>(U);                       // [Wp][H + 4]: the layer's input x (layers above the first)
  float* hr = L > 1 ? hx + (size_t)Wp * (H + 4) : hx;            // [Wp][H + 4]: the recurrent h (and g for W_pred)
  size_t hw_off = gam_rb_union_bytes(W, K, H, JH, L);
  // the LM's carve: word state, partial-word hash, lm, d, completed word id [64 + P] (A lists at buf * 32 + i, B at 64 + i), classes
  int4* mctx = nullptr;
  unsigned long long* mwh = nullptr;
  float *mlm = nullptr, *mdl = nullptr;
  int* mcw = nullptr;
  signed char* cls_sh = nullptr;
  if constexpr (LM) {
    p = U + hw_off;
    const size_t n = 64 + (size_t)P;
    mctx = reinterpret_cast<int4*>(take(n * 16));
    mwh = reinterpret_cast<unsigned long long*>(take(n * 8));
    mlm = reinterpret_cast<float*>(take(n * 4));
    mdl = reinterpret_cast<float*>(take(n * 4));
    mcw = reinterpret_cast<int*>(take(n * 4));
    cls_sh = reinterpret_cast<signed char*>(p);
    hw_off += gam_rb_lm_bytes(W, S, V);
  }
  int* hw_sh = reinterpret_cast<int*>(U + hw_off);

  int T;
  // the stream's call against its record (every thread reads the header before the first barrier; it is written behind the last)
  GamRbStreamHdr* hdr = nullptr;
  GamRbStreamEntry* ent = nullptr;
  bool begin = true;
  int maxf = 0, t0 = 0, nb0 = 1, ncount0 = 0;
  double off0 = 0.0, cb_off = 0.0, lm_off = 0.0;
  if constexpr (STREAM) {
    hdr = static_cast<GamRbStreamHdr*>(x.state);
    ent = reinterpret_cast<GamRbStreamEntry*>(hdr + 1);
    begin = (x.flags & GAM_RB_F_BEGIN) != 0;
    maxf = x.max_frames; t0 = x.t_base;
    bool ok = true;
    if (!begin) {
      ok = hdr->phase == GAM_RB_ST_BEGUN && hdr->next == x.t_base && hdr->W == W && hdr->S == S && hdr->V == V && hdr->H == H &&
           hdr->JH == JH && hdr->L == L && hdr->hw_gen == x.hw_gen && hdr->lm_gen == x.lm_gen && hdr->max_frames <= x.max_frames &&
           hdr->nb >= 0 && hdr->nb <= W && hdr->ncount >= 0;
      if (ok) {
        maxf = hdr->max_frames; t0 = hdr->t0; nb0 = hdr->nb; ncount0 = hdr->ncount;
        off0 = hdr->off; cb_off = hdr->cb_off; lm_off = hdr->lm_off;
      }
    }
    ok = ok && (long long)x.t_base + x.n - t0 <= (long long)maxf && (long long)x.t_base + x.n < 2147483648ll;
    if (!ok) {
      if (tid == 0) x.status[0] = 0;
      return;
    }
    T = x.n;
  } else {
    T = a.enc_len[b];
    T = T < 0 ? 0 : (T > Tp ? Tp : T);
    if (T == 0) {
      if constexpr (NBEST) gam_beam_emit_empty(a.nb, b, a.counts, a.score, a.logp, tid);
      else if (tid == 0) {
        a.counts[b] = 0;
        a.score[b] = 0.f;
        a.logp[b] = 0.f;
      }
      return;
    }
  }
  const int* hw = a.hw.trie;
  if (hw != nullptr && a.hw.lds) {
    for (int i = tid; i < a.hw.words; i += GAM_RB_NT) hw_sh[i] = a.hw.trie[i];
    hw = hw_sh;
  }
  float *slots, *lg;                                               // [P][SS] state slots, [Wp][LGS] logits
  Node* nodes;
  const float* encb;
  if constexpr (STREAM) {     // the slots and the nodes are the record's; the logit rows are scratch
    slots = reinterpret_cast<float*>(ent + 32);
    lg = a.ws;
    nodes = reinterpret_cast<Node*>(slots + (size_t)P * SS);
    encb = a.encp;
  } else {
    slots = a.ws + (size_t)b * a.ws_stride;
    lg = slots + (size_t)P * SS;
    nodes = a.nodes + (size_t)b * Tp * S * W;
    encb = a.encp + (size_t)b * Tp * JH;
  }

  // wave 0: rebuild the free list from the slots the A[0] list (the beam) holds
  auto rebuild_free = [&](int nb) {
    for (int i = lane; i < (P + 31) / 32; i += 64) smask[i] = 0;
    __builtin_amdgcn_wave_barrier();
    if (lane < nb) atomicOr(&smask[aslot[lane] >> 5], 1 << (aslot[lane] & 31));
    __builtin_amdgcn_wave_barrier();
    int n = 0;
    for (int base = 0; base < P; base += 64) {
      const int sl = base + lane;
      const bool fr = sl < P && !((smask[sl >> 5] >> (sl & 31)) & 1);
      const unsigned long long m = __ballot(fr);
      if (fr) freel[n + __popcll(m & ((1ull << lane) - 1ull))] = sl;
      n += __popcll(m);
    }
  };

  // ---- one predictor step for the n rows of A list `buf`: new slot aslot[i] <- LSTM(atok[i], slot apar[i]); pp = W_pred g + b_pred
  auto predict = [&](int buf, int n) {
    const int* tok = atok + buf * 32;
    const int* par = apar + buf * 32;
    const int* dst = aslot + buf * 32;
    for (int l = 0; l < L; ++l) {
      // stage the rows: recurrent h of layer l of the parent (zero for the empty y's parent -1); x = the new h of layer l - 1
      for (int e = tid; e < Wp * H; e += GAM_RB_NT) {
        const int i = e / H, k = e - i * H;
        float hv = 0.f, xv = 0.f;
        if (i < n) {
          const int ps = par[i];
          hv = ps >= 0 ? slots[(size_t)ps * SS + (size_t)l * 2 * H + k] : 0.f;
          if (l > 0) xv = slots[(size_t)dst[i] * SS + (size_t)(l - 1) * 2 * H + k];
        }
        hr[i * (H + 4) + k] = hv;
        if (l > 0) hx[i * (H + 4) + k] = xv;
      }
      __syncthreads();
      for (int jt = wave; jt * 16 < H; jt += 4) {
        const int j0 = jt * 16;
        f32x4 acc[4][2];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * rt + 4 * lg4 + r;
            const int tk = row < n ? tok[row] : V;
#pragma unroll
            for (int g = 0; g < 4; ++g)
              acc[g][rt][r] = l == 0 ? a.gate_tab[(size_t)tk * G + g * H + j0 + li] : a.bias_x[(size_t)(l - 1) * G + g * H + j0 + li];
          }
        if (l > 0) gam_rb_gates_mm<RT>(acc, hx, a.wih_x + (size_t)(l - 1) * H * G, H, j0, li, lg4);
        gam_rb_gates_mm<RT>(acc, hr, l == 0 ? a.whh_t : a.whh_x + (size_t)(l - 1) * H * G, H, j0, li, lg4);
        // the LSTM cell on the accumulators: row 16 rt + 4 q + r, hidden unit j0 + i (gate order i, f, g, o)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * rt + 4 * lg4 + r;
            if (row < n) {
              const int ps = par[row];
              const float c0 = ps >= 0 ? slots[(size_t)ps * SS + (size_t)l * 2 * H + H + j0 + li] : 0.f;
              float c2, h2;
              gam_lstm_cell<false>(acc[0][rt][r], acc[1][rt][r], acc[2][rt][r], acc[3][rt][r], c0, c2, h2);
              float* sd = slots + (size_t)dst[row] * SS + (size_t)l * 2 * H;
              sd[H + j0 + li] = c2;
              sd[j0 + li] = h2;
            }
          }
      }
      __syncthreads();
    }
    // pp = W_pred g + b_pred, g = the top layer's new h
    for (int e = tid; e < Wp * H; e += GAM_RB_NT) {
      const int i = e / H, k = e - i * H;
      hr[i * (H + 4) + k] = i < n ? slots[(size_t)dst[i] * SS + (size_t)(L - 1) * 2 * H + k] : 0.f;
    }
    __syncthreads();
    for (int ct = wave; ct * 16 < JH; ct += 4) {
      const int c0 = ct * 16;
      f32x4 acc[2];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const float bv = a.bpred[c0 + li];
        acc[rt] = (f32x4){bv, bv, bv, bv};
      }
      for (int k0 = 0; k0 < H; k0 += 16) {
        float w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = a.wpred_t[(size_t)(k0 + 4 * lg4 + e) * JH + c0 + li];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = gam_mfma4(acc[rt], gam_rc_lds4(hr + (16 * rt + li) * (H + 4) + k0 + 4 * lg4), w);
      }
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * rt + 4 * lg4 + r;
          if (row < n) slots[(size_t)dst[row] * SS + (size_t)L * 2 * H + c0 + li] = acc[rt][r];
        }
    }
    __syncthreads();
  };

  // ---- the empty hypothesis: predict(None, None) into slot 0   (STREAM without BEGIN: the record's beam instead)
  if constexpr (LM)
    for (int v = tid; v < V; v += GAM_RB_NT) cls_sh[v] = (signed char)a.lm.lm_cls[v];
  if constexpr (STREAM) {
    if (!begin && wave == 0) {
      if (lane < nb0) {
        const GamRbStreamEntry& e = ent[lane];
        ah[lane] = e.h; alen[lane] = e.len; asc[lane] = e.sc; ahn[lane] = e.hn; aacc[lane] = e.acc; acb[lane] = e.cb;
        anode[lane] = e.node; aslot[lane] = min(max(e.slot, 0), P - 1);
        if constexpr (LM) {
          mctx[lane] = e.ctx; mwh[lane] = e.wh; mlm[lane] = e.lm; mdl[lane] = e.dl; mcw[lane] = e.cw;
        }
      }
      if (lane == 0) cnt[0] = nb0;
    }
  }
  if (begin && tid == 0) {
    ah[0] = 0ull; alen[0] = 0; asc[0] = 0.f; ahn[0] = 0; aacc[0] = 0.f; acb[0] = 0.f; anode[0] = -1;
    aslot[0] = 0; atok[0] = V; apar[0] = -1;
    cnt[0] = 1;
    if constexpr (LM) {   // an empty partial word, the state <s>, lm 0
      mctx[0] = make_int4(a.lm.lm_m > 0 ? a.lm.lm_bos : -1, -1, -1, -1);
      mwh[0] = 0ull; mlm[0] = 0.f; mdl[0] = 0.f; mcw[0] = -1;
    }
  }
  __syncthreads();
  if (begin) predict(0, 1);
  if (wave == 0) rebuild_free(begin ? 1 : nb0);
  __syncthreads();

  auto brank = [&](int i) {   // rank of B entry i
    float r = bsc[i] + (bcb[i] + bacc[i]);
    if constexpr (LM) r += mlm[64 + i];
    return r;
  };
  double off = off0;       // wave 0: what the renormalisations subtracted so far
  int ncount = ncount0;    // wave 0: prefix-trie nodes of this utterance so far
  for (int t = 0; t < T; ++t) {
    int nB = 0;            // wave 0: entries of B
    int fptr = 0;          // wave 0: free slots taken this frame
    const float* et = encb + (size_t)t * JH;
    const int ts = STREAM ? x.t_base + t : t;      // the stream frame: what a node records, what the rebase goes by
    for (int s = 0; s <= S; ++s) {
      const int cur = s & 1, nx = cur ^ 1;
      const int n = cnt[cur];
      int nc = 0;          // candidates of C_s (n K, or 0 at s = S)
      if (s < S) {
        nc = n * K;
        // ---- joint rows: z = relu(encp[t] + pp), rows >= n zero
        for (int e = tid; e < Wp * JH; e += GAM_RB_NT) {
          const int i = e / JH, k = e - i * JH;
          zr[i * (JH + 4) + k] = i < n ? fmaxf(et[k] + slots[(size_t)aslot[cur * 32 + i] * SS + (size_t)L * 2 * H + k], 0.f) : 0.f;
        }
        __syncthreads();
        // ---- logits = z W_out^T + b_out: one 16-class tile per MFMA chain, W_out read once for all rows
        for (int nt = wave; nt * 16 < V; nt += 4) {
          const int v = nt * 16 + li;
          const int vc = v < V ? v : V - 1;
          const float* wr = a.wout + (size_t)vc * JH + 4 * lg4;
          f32x4 acc[2];
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
          for (int k0 = 0; k0 < JH; k0 += 16) {
            const f32x4 wf = *reinterpret_cast<const f32x4*>(wr + k0);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt] = gam_mfma4(acc[rt], gam_rc_lds4(zr + (16 * rt + li) * (JH + 4) + k0 + 4 * lg4), wf);
          }
          if (v < V) {
            const float bo = a.bout[v];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int row = 16 * rt + 4 * lg4 + r;
                if (row < n) lg[(size_t)row * LGS + v] = acc[rt][r] + bo;
              }
          }
        }
        __syncthreads();
        // ---- one wave per row: log-sum-exp, blank, the top K -> the candidates of C_s
        const int nrv = (V + 63) >> 6;
        for (int r = wave; r < n; r += 4) {
          const float* xr = lg + (size_t)r * LGS;
          float x[GAM_BEAM_RPL];
          float mx = -INFINITY;
#pragma unroll
          for (int j = 0; j < GAM_BEAM_RPL; ++j) {
            const int v = lane + 64 * j;
            x[j] = (j < nrv && v < V) ? xr[v] : -INFINITY;
            mx = fmaxf(mx, x[j]);
          }
          mx = gam_wave_max(mx);
          float se = 0.f;
#pragma unroll
          for (int j = 0; j < GAM_BEAM_RPL; ++j)
            if (j < nrv) se += expf(x[j] - mx);
          se = gam_wave_sum(se);
          const float lse = mx + logf(se);
          unsigned long long k[GAM_BEAM_RPL];
#pragma unroll
          for (int j = 0; j < GAM_BEAM_RPL; ++j) {
            const int v = lane + 64 * j;
            k[j] = (j < nrv && v < V - 1) ? (((unsigned long long)gam_beam_ord(x[j]) << 32) | (unsigned)(0xffff - v)) : 0ull;
          }
          unsigned long long out;
          gam_beam_wave_topn(k, nrv, K, lane, out);
          const int o = cur * 32 + r;
          if (lane == 0) rlpb[r] = xr[blank] - lse;
          if (lane < K) {
            const int v = 0xffff - (int)(out & 0xffff);
            const float sc = asc[o] + (gam_beam_unord((unsigned)(out >> 32)) - lse);
            int hn = ahn[o];
            float acc = aacc[o], cb = acb[o];
            if (hw != nullptr) gam_beam_hw_step(hw, a.hw.nodes, a.hw.beta, v, hn, acc, cb);
            float rank = sc + (cb + acc);
            if constexpr (LM) {   // a's lm, plus d(a) when v completes a's partial word
              float lmv = mlm[o];
              if (cls_sh[v] != 0 && mwh[o] != 0ull) lmv += mdl[o];
              rank += lmv;
            }
            const int q = r * K + lane;
            const int key = r * GAM_BEAM_KEY_STRIDE + v + 1;
            ckey[q] = rank > -INFINITY ? gam_beam_key(gam_beam_ord(rank), key, q) : 0ull;
            csc[q] = sc;
            cacc[q] = acc;
            ccb[q] = cb;
            chn[q] = hn;
          }
        }
        __syncthreads();
      }
      if (wave == 0) {
        // ---- blank candidates (s < S) or forced advances (s = S) of A_s into B
        {
          const int o = cur * 32 + lane;
          const bool act = lane < n;
          const float sc = act ? (s < S ? asc[o] + rlpb[lane] : asc[o]) : -INFINITY;
          const unsigned long long h = act ? ah[o] : 0ull;
          const int len = act ? alen[o] : -1;
          int f = -1;
          for (int i = 0; i < nB; ++i)
            if (f < 0 && blen[i] == len && bh[i] == h) f = i;
          const bool valid = act && sc > -INFINITY;
          if (valid && f >= 0) {
            bsc[f] = gam_beam_lse(bsc[f], sc);
            if (sc > bcs[f]) {
              bcs[f] = sc;
              bslot[f] = aslot[o];
              bnode[f] = anode[o];
            }
          }
          const bool add = valid && f < 0;
          const unsigned long long m = __ballot(add);
          if (add) {
            const int d = nB + __popcll(m & ((1ull << lane) - 1ull));
            bh[d] = h; blen[d] = len; bsc[d] = sc; bcs[d] = sc; bkey[d] = s * 32 + lane;
            bslot[d] = aslot[o]; bnode[d] = anode[o]; bhn[d] = ahn[o]; bacc[d] = aacc[o]; bcb[d] = acb[o];
            if constexpr (LM) {
              mctx[64 + d] = mctx[o]; mwh[64 + d] = mwh[o]; mlm[64 + d] = mlm[o]; mdl[64 + d] = mdl[o]; mcw[64 + d] = mcw[o];
            }
          }
          nB += __popcll(m);
        }
        // ---- theta, then A_{s+1} = top W of the candidates above it
        int ns = 0;
        if (nc > 0) {
          unsigned ord_theta = 0u;     // (every finite or +inf rank orders above it)
          unsigned long long k[GAM_BEAM_RPL];
          if (nB >= W) {
            const int nr = (nB + 63) >> 6;
#pragma unroll
            for (int j = 0; j < GAM_BEAM_RPL; ++j) {
              const int i = lane + 64 * j;
              k[j] = (j < nr && i < nB) ? gam_beam_key(gam_beam_ord(brank(i)), bkey[i], i) : 0ull;
            }
            unsigned long long sel;
            gam_beam_wave_topn(k, nr, W, lane, sel);
            ord_theta = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(sel >> 32), W - 1);
          }
          const int nr = (nc + 63) >> 6;
#pragma unroll
          for (int j = 0; j < GAM_BEAM_RPL; ++j) {
            const int q = lane + 64 * j;
            const unsigned long long kq = (j < nr && q < nc) ? ckey[q] : 0ull;
            k[j] = (unsigned)(kq >> 32) > ord_theta ? kq : 0ull;
          }
          unsigned long long sel;
          ns = gam_beam_wave_topn(k, nr, W, lane, sel);
          if (lane < ns) {
            const int q = (int)(sel & 0xffff);
            const int r = q / K;
            const int key = 0xffff - (int)((sel >> 16) & 0xffff);
            const int v = key - r * GAM_BEAM_KEY_STRIDE - 1;
            const int o = cur * 32 + r, d = nx * 32 + lane;
            const int idx = ncount + lane;
            if constexpr (STREAM) nodes[idx] = make_int4(anode[o], v, ts, 0);
            else nodes[idx] = make_int2(anode[o], (v << 13) | t);
            ah[d] = ah[o] * GAM_BEAM_HASH_P + (unsigned long long)(v + 1);
            alen[d] = alen[o] + 1;
            asc[d] = csc[q];
            ahn[d] = chn[q]; aacc[d] = cacc[q]; acb[d] = ccb[q];
            anode[d] = idx;
            aslot[d] = freel[fptr + lane];
            atok[d] = v;
            apar[d] = aslot[o];
            if constexpr (LM) {   // the new entry's LM state; a non-empty partial word queries d and its word id
              const unsigned long long wh = mwh[o];
              const int4 cx = mctx[o];
              const int cl = cls_sh[v];
              const bool done = cl != 0 && wh != 0ull;      // v completes a's partial word
              const int4 ncx = done ? make_int4(mcw[o], cx.x, cx.y, cx.z) : cx;
              const unsigned long long nwh =
                  cl == 0 ? wh * GAM_BEAM_HASH_P + (unsigned long long)(v + 1) : (cl == 1 ? (unsigned long long)(v + 1) : 0ull);
              int w = -1;
              float dl = 0.f;
              if (nwh != 0ull) dl = a.lm.lm_alpha * gam_lm_query(a.lm, true, nwh, w, ncx) + a.lm.lm_beta;
              mlm[d] = done ? mlm[o] + mdl[o] : mlm[o];
              mctx[d] = ncx; mwh[d] = nwh; mdl[d] = dl; mcw[d] = w;
            }
          }
          ncount += ns;
          fptr += ns;
        }
        if (lane == 0) cnt[nx] = ns;
      }
      __syncthreads();
      const int nn = cnt[nx];
      if (nn == 0) break;
      predict(nx, nn);
    }
    // ---- the new beam: top W of B -> A list 0, renormalised; the free list from its slots
    if (wave == 0) {
      unsigned long long k[GAM_BEAM_RPL];
      const int nr = (nB + 63) >> 6;
#pragma unroll
      for (int j = 0; j < GAM_BEAM_RPL; ++j) {
        const int i = lane + 64 * j;
        k[j] = (j < nr && i < nB) ? gam_beam_key(gam_beam_ord(brank(i)), bkey[i], i) : 0ull;
      }
      unsigned long long sel;
      const int nb = gam_beam_wave_topn(k, nr, W, lane, sel);
      if (nb > 0) {
        float M = gam_beam_unord((unsigned)__builtin_amdgcn_readlane((int)(unsigned)(sel >> 32), 0));
        if constexpr (LM) M -= mlm[64 + __builtin_amdgcn_readlane((int)(sel & 0xffff), 0)];     // (scores keep O(one frame))
        off += (double)M;
        float cb0 = 0.f, lm0 = 0.f;      // STREAM, at a rebase frame: the best kept entry's committed bonus and LM term leave every entry's
        if constexpr (STREAM) {
          if (ts > 0 && (ts & (GAM_RB_STREAM_REBASE - 1)) == 0) {
            const int i0 = __builtin_amdgcn_readlane((int)(sel & 0xffff), 0);
            cb0 = bcb[i0];
            cb_off += (double)cb0;
            if constexpr (LM) {
              lm0 = mlm[64 + i0];
              lm_off += (double)lm0;
            }
          }
        }
        if (lane < nb) {
          const int i = (int)(sel & 0xffff);
          ah[lane] = bh[i]; alen[lane] = blen[i]; asc[lane] = bsc[i] - M;
          ahn[lane] = bhn[i]; aacc[lane] = bacc[i]; acb[lane] = STREAM ? bcb[i] - cb0 : bcb[i];
          anode[lane] = bnode[i]; aslot[lane] = bslot[i];
          if constexpr (LM) {
            mctx[lane] = mctx[64 + i]; mwh[lane] = mwh[64 + i]; mlm[lane] = STREAM ? mlm[64 + i] - lm0 : mlm[64 + i];
            mdl[lane] = mdl[64 + i]; mcw[lane] = mcw[64 + i];
          }
        }
      }
      if (lane == 0) cnt[0] = nb;
      __builtin_amdgcn_wave_barrier();
      rebuild_free(nb);
    }
    __syncthreads();
    if (cnt[0] == 0) break;      // (every candidate -inf: cannot happen with finite log-probs)
  }

  // ---- final pick (pending hotword bonus dropped; with the LM the last word and </s> added), backtrack
  if (wave == 0) {
    const int nb = cnt[0];
    if constexpr (STREAM) {
      // ---- store the record: all 32 entries (zeros beyond the beam), then the header
      if (lane < 32) {
        GamRbStreamEntry e;
        memset(&e, 0, sizeof e);
        if (lane < nb) {
          e.h = ah[lane]; e.len = alen[lane]; e.sc = asc[lane]; e.hn = ahn[lane]; e.acc = aacc[lane]; e.cb = acb[lane];
          e.node = anode[lane]; e.slot = aslot[lane];
          if constexpr (LM) {
            e.wh = mwh[lane]; e.ctx = mctx[lane]; e.lm = mlm[lane]; e.dl = mdl[lane]; e.cw = mcw[lane];
          }
        }
        ent[lane] = e;
      }
      const bool end = (x.flags & GAM_RB_F_END) != 0;
      if (lane == 0) {
        hdr->phase = end ? GAM_RB_ST_ENDED : GAM_RB_ST_BEGUN;
        hdr->W = W; hdr->S = S; hdr->V = V; hdr->H = H; hdr->JH = JH; hdr->L = L;
        hdr->hw_gen = x.hw_gen; hdr->lm_gen = x.lm_gen;
        hdr->nb = nb; hdr->ncount = ncount;
        hdr->next = x.t_base + x.n; hdr->max_frames = maxf; hdr->t0 = t0;
        hdr->pad0[0] = hdr->pad0[1] = 0;
        hdr->off = off; hdr->cb_off = cb_off; hdr->lm_off = lm_off;
        for (int i = 0; i < 10; ++i) hdr->pad1[i] = 0;
        x.status[0] = 1;
      }
      if (!end) return;
      if (x.t_base + x.n == t0) {      // a stream without a frame
        if (lane == 0) {
          a.counts[0] = 0;
          x.score[0] = 0.0;
          x.logp[0] = 0.0;
        }
        return;
      }
    }
    float val = lane < nb ? asc[lane] + acb[lane] : -INFINITY;
    float lmf = 0.f;
    if constexpr (LM) {
      if (lane < nb) {
        int4 cx = mctx[lane];
        lmf = mlm[lane];
        if (mwh[lane] != 0ull) {
          lmf += mdl[lane];
          cx = make_int4(mcw[lane], cx.x, cx.y, cx.z);
        }
        int w = a.lm.lm_eos;
        lmf += a.lm.lm_alpha * gam_lm_query(a.lm, false, 0ull, w, cx);
        val += lmf;
      }
    }
    if constexpr (NBEST) {   // the nb.n best entries instead of the best one (gam_search.h): the same value, key and arithmetic
      const double lp_ = (double)(lane < nb ? asc[lane] : -INFINITY) + off;
      const float sc = lane < nb ? (LM ? (float)(lp_ + (double)acb[lane] + (double)lmf) : (float)(lp_ + (double)acb[lane])) : -INFINITY;
      gam_beam_emit_nbest(a.nb, b, a.cap, lane < nb, val, sc, (float)lp_, lane < nb ? alen[lane] : 0, lane < nb ? anode[lane] : -1, nodes,
                          a.ids, a.frames, a.counts, a.score, a.logp, lane);
      return;
    }
    const unsigned long long key = lane < nb ? (((unsigned long long)gam_beam_ord(val) << 32) | (unsigned)(0xffff - lane)) : 0ull;
    const unsigned long long m = gam_beam_wave_max(key);
    const int best = m ? 0xffff - (int)(m & 0xffff) : -1;
    if (best < 0) {
      if (lane == 0) {
        a.counts[b] = 0;
        if constexpr (STREAM) {
          x.score[0] = -(double)INFINITY;
          x.logp[0] = -(double)INFINITY;
        } else {
          a.score[b] = -INFINITY;
          a.logp[b] = -INFINITY;
        }
      }
    } else if (lane == best) {
      const double lp_ = (double)asc[lane] + off;
      if constexpr (STREAM) {      // fp64, with what the rebases took out
        x.logp[0] = lp_;
        x.score[0] = (LM ? lp_ + (double)acb[lane] + (double)lmf : lp_ + (double)acb[lane]) + cb_off + lm_off;
      } else {
        a.logp[b] = (float)lp_;
        if constexpr (LM) a.score[b] = (float)(lp_ + (double)acb[lane] + (double)lmf);
        else a.score[b] = (float)(lp_ + (double)acb[lane]);
      }
      const int n = alen[lane] < a.cap ? alen[lane] : a.cap;
      a.counts[b] = n;
      int* ids = a.ids + (size_t)b * a.cap;
      int* fr = a.frames + (size_t)b * a.cap;
      int node = anode[lane];
      for (int i = alen[lane] - 1; i >= 0; --i) {
        const Node e = nodes[node];
        if (i < n) {
          if constexpr (STREAM) {
            ids[i] = e.y;
            fr[i] = e.z;
          } else {
            ids[i] = e.y >> 13;
            fr[i] = e.y & 8191;
          }
        }
        node = e.x;
      }
    }
  }
}
