// gam_search.h -- what the CTC prefix beam search (gam_beam.h) and the RNN-T beam search (gam_rnnt_beam.h) share: limits, the
// hotword and LM argument blocks, log-add-exp, orderable selection keys, the wave top-n, the hotword trie walk, the n-gram LM query and the N-best emission.
// Every function is __forceinline__: left to the inliner, a body became a call that copied the argument struct to scratch
// (DESIGN.md 4.12).
//
// Hypothesis identity: (length, 64-bit polynomial hash h(y + c) = h(y) * P + c + 1).  A collision would merge two different
// hypotheses; it is accepted (2^-64 per compare) and the references, with real tuples, cannot show one.
//
// Hotwords: a trie of token-id phrases with one boost beta per matched token.  Only an extension by c moves an entry's state
// (node, acc): to node's child for c (acc += beta; at a phrase end acc is committed and reset; the walk stays on the child if it has
// children, else returns to the root), else the pending acc is rolled back and the walk restarts from the root's child for c.
// There are no failure links: with the phrase "a a b", the text "a a a b" is not boosted -- the third "a" finds no child of "a a",
// rolls back and restarts at "a", then "b" is no child of "a".  bonus = committed + acc; the state depends on y alone, so merged
// candidates agree on it.  The final pick drops the pending acc.
// Hotword trie: CSR -- offsets [n_nodes + 1], then edges (token | end << 11 | child << 12) sorted by token per node, searched by
// binary search; copied to LDS when it fits (GAM_BEAM_HW_LDS_MAX bytes), else read from global memory (L2-resident).
// Limits (host errors beyond them): W <= 32, V <= 1025, <= 1024 phrases, <= 16384 phrase tokens.
//
// Word n-gram LM (gigaam_amd/lm.py builds the tables).  Every token has a class: 0 continues the current word, 1 starts a new word
// (a SentencePiece piece beginning with U+2581; the token belongs to the new word), 2 is a separator (the " " of a char-wise
// vocabulary; it belongs to no word).  An entry's partial word is its token ids since the last class-1/2 token, identified by the
// spelling hash wh = h(ids) (h as for hypotheses, from 0; 0 = empty); its LM state is the word ids of its last order - 1 completed
// words (<s> at the start).  An extension of y by a class-1/2 token completes y's partial word w when it is non-empty: the entry's
// `lm` grows by d(y) = alpha ln P(w | state) + beta and w enters the state; class 0 appends the token to the partial word, class 1
// starts the partial word [token], class 2 leaves it empty.  P is ARPA back-off (natural log; a word outside the
// word table is <unk>, which scores unk_logp when the ARPA has no <unk> unigram).  Partial words are not scored.  All of it depends
// on y alone, so merged candidates agree on it.  Final pick: the last partial word is completed, then
// alpha ln P(</s> | state) is added.
//   Cost: one LM query per NEW entry, not per candidate -- d(y) and w's id are the same whichever boundary token completes w, so
//   they are queried once when y enters a beam and the candidate phase only adds them.  A query is two rounds of global loads
//   (the tables stay L2 / Infinity-Cache resident): the word (word table) together with the back-off weights of the state's suffixes
//   (n-gram table; their keys are known before the word id), then the n-grams (suffix, w) of every order together.
// Tables: 16-byte slots {u64 key, 2 x 32 bit} (word table: word id; n-gram table: ln p, ln back-off as f32), open addressing,
// linear probing, a power-of-two slot count < 2^30, load <= 0.5; key = mix64(h) (splitmix64 finaliser, 0 -> 1), 0 = free slot;
// n-gram h = n, then h = h * P + (id + 1) per word, oldest first.  A probe reads at most the host's longest chain.  Full 64-bit keys
// are compared: a collision is accepted (2^-64 per compare), as for hypotheses.  Limits: order <= 5.
#pragma once
#include <stddef.h>
#include "gam_common.h"

#define GAM_BEAM_MAX_W 32
#define GAM_BEAM_MAX_V 1025
#define GAM_BEAM_RPL 17                  // values per lane: ceil(max(1025, 32 * 33) / 64)
#define GAM_BEAM_MAX_PHRASES 1024
#define GAM_BEAM_MAX_HW_TOKENS 16384
#define GAM_BEAM_HW_LDS_MAX (64 * 1024)
#define GAM_BEAM_KEY_STRIDE 1026         // origin key = source position * 1026 + (stay ? 0 : c + 1), < 2^16
#define GAM_BEAM_HASH_P 0x100000001b3ull
#define GAM_BEAM_LM_MAX_ORDER 5

struct GamHwArgs {
  const int* trie;       // hotword trie (NULL: none): offsets [nodes + 1] | edges
  int nodes, words, lds; // trie nodes, ints at `trie`, whether the kernel copies it to LDS
  float beta;
};

struct GamLmArgs {       // the n-gram LM (the <true> kernels only)
  const int* lm_cls;     // [V] token classes
  const uint4* lm_wt;    // word table slots
  const uint4* lm_ng;    // n-gram table slots
  int lm_wmask, lm_wprobe, lm_nmask, lm_nprobe;   // slots - 1, longest probe chain
  int lm_m, lm_bos, lm_eos, lm_unk;               // order - 1, word ids
  float lm_unk_logp, lm_alpha, lm_beta;
};
static_assert(sizeof(GamHwArgs) == 24 && offsetof(GamHwArgs, beta) == 20 && sizeof(GamLmArgs) == 72 &&
              offsetof(GamLmArgs, lm_wmask) == 24 && offsetof(GamLmArgs, lm_beta) == 64, "hotword / LM argument blocks");

__device__ __forceinline__ float gam_beam_lse(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + gam_fast_log(1.0f + gam_fast_exp(fminf(a, b) - m));
}
__device__ __forceinline__ unsigned gam_beam_ord(float f) {     // float -> unsigned, order preserving
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gam_beam_unord(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
// Selection key: orderable rank bits (gam_beam_ord) | 0xffff - origin key | index, so that equal ranks go to the smaller origin key.
__device__ __forceinline__ unsigned long long gam_beam_key(unsigned rank_ord, int key, int q) {
  return ((unsigned long long)rank_ord << 32) | ((unsigned)(0xffff - key) << 16) | (unsigned)q;
}

// Wave maximum of a 64-bit key by DPP (the pattern of gam_dpp_wave_max on both halves), read from lane 63: uniform.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long gam_beam_dpp_max(unsigned long long v) {
  const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
  const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
  const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
  const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
  return o > v ? o : v;
}
__device__ __forceinline__ unsigned long long gam_beam_wave_max(unsigned long long v) {
  v = gam_beam_dpp_max<0xb1, 0xf>(v);
  v = gam_beam_dpp_max<0x4e, 0xf>(v);
  v = gam_beam_dpp_max<0x141, 0xf>(v);
  v = gam_beam_dpp_max<0x140, 0xf>(v);
  v = gam_beam_dpp_max<0x142, 0xa>(v);
  v = gam_beam_dpp_max<0x143, 0xc>(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

// The n largest of the keys k[0..nr) of the wave (n <= 64, keys unique or 0): the i-th largest lands in lane i's `out`.  Returns
// how many non-zero keys were found (<= n).
__device__ __forceinline__ int gam_beam_wave_topn(unsigned long long (&k)[GAM_BEAM_RPL], int nr, int n, int lane,
                                                  unsigned long long& out) {
  unsigned long long loc = 0;
#pragma unroll
  for (int r = 0; r < GAM_BEAM_RPL; ++r)
    if (r < nr) loc = k[r] > loc ? k[r] : loc;
  int found = 0;
  out = 0;
  for (; found < n; ++found) {
    const unsigned long long m = gam_beam_wave_max(loc);
    if (m == 0) break;
    if (lane == found) out = m;
    loc = 0;
#pragma unroll
    for (int r = 0; r < GAM_BEAM_RPL; ++r) {
      if (r < nr) {
        if (k[r] == m) k[r] = 0;
        loc = k[r] > loc ? k[r] : loc;
      }
    }
  }
  return found;
}

// Edge of hotword node `node` for token c (edges sorted by token), or -1.
__device__ __forceinline__ int gam_beam_hw_find(const int* hw, int n_nodes, int node, int c) {
  const int* E = hw + n_nodes + 1;
  int lo = hw[node];
  const int end = hw[node + 1];
  int hi = end;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((E[mid] & 2047) < c) lo = mid + 1;
    else hi = mid;
  }
  return (lo < end && (E[lo] & 2047) == c) ? E[lo] : -1;
}

// The hotword state after an extension by c.
__device__ __forceinline__ void gam_beam_hw_step(const int* hw, int n_nodes, float beta, int c, int& node, float& acc, float& cb) {
  int e = gam_beam_hw_find(hw, n_nodes, node, c);
  if (e < 0 && node != 0) {          // roll back the pending part, restart from the root
    acc = 0.f;
    node = 0;
    e = gam_beam_hw_find(hw, n_nodes, 0, c);
  }
  if (e < 0) {                       // (at the root acc is 0)
    node = 0;
    acc = 0.f;
    return;
  }
  acc += beta;
  const int child = e >> 12;
  if ((e >> 11) & 1) {
    cb += acc;
    acc = 0.f;
  }
  node = hw[child + 1] > hw[child] ? child : 0;
}

// ---- the n-gram LM
__device__ __forceinline__ unsigned long long gam_lm_mix(unsigned long long x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x ? x : 1ull;
}

// Linear probes of up to NQ keys at once (bit q of `live`: query q runs; query 0 in table t0 of mask m0, the others in t of mask
// m); every round issues the loads of all open queries before it compares any.  Returns the found bits; val[q] is the found slot's
// third word (q == 0 or !FOURTH) or its fourth.
template <int NQ, bool FOURTH>
__device__ __forceinline__ unsigned gam_lm_probe(const uint4* t0, int m0, const uint4* t, int m, int maxp,
                                                 const unsigned long long (&key)[NQ], unsigned live, unsigned (&val)[NQ]) {
  unsigned open = live, found = 0;
  for (int i = 0; i < maxp && open; ++i) {
    uint4 e[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const unsigned sl = (unsigned)(key[q] + (unsigned)i) & (unsigned)(q == 0 ? m0 : m);
      e[q] = ((open >> q) & 1) ? (q == 0 ? t0 : t)[sl] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const unsigned long long k = ((unsigned long long)e[q].y << 32) | e[q].x;
      const bool hit = ((open >> q) & 1) && k == key[q];
      if (hit) found |= 1u << q;
      val[q] = hit ? ((FOURTH && q != 0) ? e[q].w : e[q].z) : val[q];
      if (hit || k == 0ull) open &= ~(1u << q);
    }
  }
  return found;
}

// ln P(w | s) by ARPA back-off, s = (s.x most recent, s.y, s.z, s.w), -1 = no word; the first lm_m of them are the context.  With
// `word`, w is the word table's id for spelling hash wh (lm_unk when it has none).  Returns ln P and sets w.
__device__ __forceinline__ float gam_lm_query(const GamLmArgs& a, bool word, unsigned long long wh, int& w, int4 s4) {
  constexpr int NQ = GAM_BEAM_LM_MAX_ORDER;
  const int m = a.lm_m;
  const int s[4] = {s4.x, s4.y, s4.z, s4.w};
  // round A: the word (slot 0, word table), and the back-off contexts B_k = (s[k-1] .. s[0]), k = 1..m (slot k, n-gram table)
  unsigned long long kA[NQ];
  unsigned vA[NQ] = {0, 0, 0, 0, 0};
  unsigned live = word ? 1u : 0u;
  kA[0] = gam_lm_mix(wh);
#pragma unroll
  for (int k = 1; k < NQ; ++k) {
    unsigned long long h = (unsigned long long)k;
#pragma unroll
    for (int i = k - 1; i >= 0; --i) h = h * GAM_BEAM_HASH_P + (unsigned long long)(s[i] + 1);
    kA[k] = gam_lm_mix(h);
    if (k <= m && s[k - 1] >= 0) live |= 1u << k;
  }
  const unsigned fA = gam_lm_probe<NQ, true>(a.lm_wt, a.lm_wmask, a.lm_ng, a.lm_nmask, max(a.lm_wprobe, a.lm_nprobe), kA, live, vA);
  if (word) w = (fA & 1) ? (int)vA[0] : a.lm_unk;
  // round B: the n-grams P_k = (s[k-1] .. s[0], w), k = 0..m
  unsigned long long kB[NQ];
  unsigned vB[NQ] = {0, 0, 0, 0, 0};
  live = 0;
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    unsigned long long h = (unsigned long long)(k + 1);
#pragma unroll
    for (int i = k - 1; i >= 0; --i) h = h * GAM_BEAM_HASH_P + (unsigned long long)(s[i] + 1);
    h = h * GAM_BEAM_HASH_P + (unsigned long long)(w + 1);
    kB[k] = gam_lm_mix(h);
    if (k <= m && (k == 0 || s[k - 1] >= 0)) live |= 1u << k;
  }
  const unsigned fB = gam_lm_probe<NQ, false>(a.lm_ng, a.lm_nmask, a.lm_ng, a.lm_nmask, a.lm_nprobe, kB, live, vB);
  // the longest context that has (context, w), plus the back-offs of the longer ones; no unigram: unk_logp
  float bo = 0.f, lp = a.lm_unk_logp;
  bool got = false;
#pragma unroll
  for (int k = NQ - 1; k >= 0; --k) {
    if (!got && ((fB >> k) & 1)) {
      lp = __uint_as_float(vB[k]) + bo;
      got = true;
    }
    if (!got && k >= 1 && ((fA >> k) & 1)) bo += __uint_as_float(vA[k]);
  }
  return lp;
}

// ---- N-best emission (gam_ctc_beam_nbest / gam_rnnt_beam_nbest): what the <.., true> kernels run in place of the 1-best pick.
// The kernels' ids / frames are then [B, n, cap] and counts / score / logp [B, n]; rows r >= n_hyp[b] get counts 0 and score =
// logp = -inf (their ids / frames are not written).
struct GamNbestArgs {
  int* n_hyp;            // [B] hypotheses written (NULL in the 1-best calls)
  int n, pad;            // hypotheses asked for, 1 <= n <= W
};
static_assert(sizeof(GamNbestArgs) == 16, "N-best argument block");

// Wave 0 after the last frame.  Lane i holds entry i of the final beam: `live`, its ranking value `val` (what the 1-best pick ranks
// by), its rounded score and logp, its token count and prefix-trie node.  The nb.n best by (val descending, position ascending) --
// the 1-best pick's key -- are written in that order: lane r fetches hypothesis r from its lane and backtracks it, the lanes in
// parallel.  Row 0 is therefore the 1-best result bit for bit.
__device__ __forceinline__ void gam_beam_emit_nbest(const GamNbestArgs& nb, int b, int cap, bool live, float val, float score, float logp,
                                                    int len, int node, const int2* nodes, int* ids, int* frames, int* counts, float* oscore,
                                                    float* ologp, int lane) {
  unsigned long long k[GAM_BEAM_RPL];
#pragma unroll
  for (int r = 0; r < GAM_BEAM_RPL; ++r) k[r] = 0ull;
  k[0] = live ? (((unsigned long long)gam_beam_ord(val) << 32) | (unsigned)(0xffff - lane)) : 0ull;
  unsigned long long sel;
  const int nh = gam_beam_wave_topn(k, 1, nb.n, lane, sel);
  const int src = lane < nh ? 0xffff - (int)(sel & 0xffff) : lane;
  score = __shfl(score, src);
  logp = __shfl(logp, src);
  len = __shfl(len, src);
  node = __shfl(node, src);
  if (lane == 0) nb.n_hyp[b] = nh;
  if (lane >= nb.n) return;
  const size_t row = (size_t)b * nb.n + lane;
  if (lane >= nh) {
    counts[row] = 0;
    oscore[row] = -INFINITY;
    ologp[row] = -INFINITY;
    return;
  }
  const int n = len < cap ? len : cap;
  counts[row] = n;
  oscore[row] = score;
  ologp[row] = logp;
  int* oi = ids + row * cap;
  int* of = frames + row * cap;
  for (int i = len - 1; i >= 0; --i) {
    const int2 e = nodes[node];
    if (i < n) {
      oi[i] = e.y >> 13;
      of[i] = e.y & 8191;
    }
    node = e.x;
  }
}
// enc_len[b] = 0: one empty hypothesis with score = logp = 0 (threads tid < nb.n of the workgroup).
__device__ __forceinline__ void gam_beam_emit_empty(const GamNbestArgs& nb, int b, int* counts, float* score, float* logp, int tid) {
  if (tid == 0) nb.n_hyp[b] = 1;
  if (tid < nb.n) {
    const size_t row = (size_t)b * nb.n + tid;
    counts[row] = 0;
    score[row] = tid == 0 ? 0.f : -INFINITY;
    logp[row] = tid == 0 ? 0.f : -INFINITY;
  }
}
