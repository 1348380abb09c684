// gam_beam.h -- CTC prefix beam search with hotword boosting (gam_ctc_beam / gam_op_ctc_beam).
//
// The algorithm (shared with tests/ctc_beam_ref.py, which holds real prefix tuples): for utterance b with log-probs lp[t, v]
// (t < T = enc_len[b], blank = V - 1), beam width W and K = min(W, V - 1) candidate tokens per frame (the top-K non-blank ids of
// lp[t], ties to the lower id), every beam entry y (last token l; p_b / p_nb: log-probs of the paths ending in blank / non-blank)
// contributes, with (+) = log-add-exp:
//   stay    y.p_b      (+)= (p_b (+) p_nb) + lp[t, blank]
//   repeat  y.p_nb     (+)= p_nb + lp[t, l]                             (y non-empty, whether or not l is a candidate)
//   extend  (y+c).p_nb (+)= (c == l ? p_b : p_b (+) p_nb) + lp[t, c]   for each candidate c
// Candidates naming the same prefix merge -- the only way two can is an extension y_j + c that equals another entry y_i; if that
// extension's term outweighs the entry's own stay + repeat mass, the prefix's last token re-enters the beam at t (its frame becomes t,
// so a token's frame is where the dominant extension entered: the first frame of its run on the best path).  The new
// beam is the top W by rank = (p_b (+) p_nb) + bonus; equal ranks go by the origin key (source entry's position, -1 for stay /
// repeat else c) ascending, a merged prefix taking its smaller key.  Candidates of rank -inf are dropped.
//
// Hotwords: the rules and the trie of gam_search.h.  The final pick drops the pending acc: best (p_b (+) p_nb) + committed, ties to the
// lower beam position.
//
// Shape: one workgroup of GAM_BEAM_NT threads per utterance, t the sequential loop, TWO barriers per frame:
//   phase 1 (every thread)  one candidate per thread and step: stay / repeat of entry j (q = j (K + 1) + K) or the extension of
//                            entry j by the s-th top-K id (q = j (K + 1) + s); its rank, origin key and index packed into one
//                            64-bit key (orderable rank bits | 0xffff - origin | q), 0 for no candidate.          -- barrier A
//   phase 2 (wave 0)        top W of the <= W (K + 1) <= 1056 keys: each lane holds <= 17 in registers; W wave maxima (DPP),
//                            the winner removed each time.  Then the new beam: lane i builds entry i, extensions get a prefix-trie
//                            node, and each entry finds its parent prefix in the new beam (a hash compare per entry: O(W))
//                            -- the child masks with which phase 1 finds merges.
//           (wave 1)        the top K of frame t + 1 (the same wave maxima over the row, <= 17 values per lane), and the row
//                            itself into LDS (blank and repeat terms); the row of frame t + 2 is loaded meanwhile.  -- barrier B
// Prefix identity: (length, 64-bit hash), gam_search.h.
// Precision: every frame subtracts the best kept rank from p_b / p_nb and adds it to an fp64 offset, so the stored values stay
// O(one frame's log-probs); the log-add-exp runs on the hardware transcendentals (gam_fast_exp / gam_fast_log, ~1 ulp).
// Prefix trie: only surviving extensions (and re-entries) create a node {parent, token << 13 | frame}, in a grow-only handle workspace of
// B x T' x W nodes (at most W per frame).  The backtrack runs in the same kernel and writes ids / frames / count / score / logp.
// Limits (host errors beyond them): those of gam_search.h and T' <= GAM_ALIGN_MAX_T.
//
// N-best (template <bool NBEST>; gam_ctc_beam_nbest): the final pick becomes gam_search.h's emission of the n best entries of the
// final beam; everything before it is the same code.
//
// Word n-gram LM (template <bool LM>; gam_ctc_beam_kernel<false> is the kernel without it, unchanged; tests/ctc_beam_ref.py with an
// LMSpec is the float64 reference).  The word rules, the cost split and the tables of gam_search.h, applied to prefixes:
// rank = (p_b (+) p_nb) + bonus + lm.  Final pick: best (p_b (+) p_nb) + committed + lm with the last word and </s> added.
// score = log p + committed + lm; logp is unchanged.  Wave 0 computes d and the word id in phase 2 for each new entry whose partial
// word changed (an extension; a stay keeps its entry's) and phase 1 only adds them.  Renormalisation subtracts the best rank minus its
// lm, so p_b / p_nb stay O(one frame) however large lm grows.
#pragma once
#include "gam_search.h"

#define GAM_BEAM_NT 256

struct GamBeamArgs {
  const float* lp;       // [B, Tp, V] log-probs
  const int* enc_len;    // [B]
  int Tp, V, W, K;
  GamHwArgs hw;
  int2* nodes;           // [B, Tp * W] prefix-trie nodes
  int* ids;              // [B, Tp]
  int* frames;           // [B, Tp]
  int* counts;           // [B]
  float* score;          // [B]
  float* logp;           // [B]
  GamLmArgs lm;
  GamNbestArgs nb;       // the <.., true> kernels only: ids / frames are then [B, n, Tp], counts / score / logp [B, n]
};
// (the kernel argument layout the fields had before the two blocks were structs of their own; the N-best block is appended)
static_assert(sizeof(GamBeamArgs) == 192 && offsetof(GamBeamArgs, hw) == 32 && offsetof(GamBeamArgs, nodes) == 56 &&
              offsetof(GamBeamArgs, lm) == 104 && offsetof(GamBeamArgs, nb) == 176, "GamBeamArgs layout");

// LDS carve (host and device): beam state [2][32] (hash, parent hash: u64; p_b, p_nb, acc, committed: f32; len, last, prefix node,
// hotword node, parent, child mask: i32), top-K ids / values [2][32], beam sizes, candidate keys u64 [NC], candidate p_b, p_nb, acc,
// committed, hotword node [NC], the emission row [V], the hotword trie when it lies in LDS; with the LM, from the next 16-byte
// boundary: beam LM state [2][32] (partial-word hash u64, state int4, lm, d, completed word id), top-K classes [2][32], classes [V] i8.
__host__ __device__ static inline size_t gam_beam_lds_base(int W, int K, int V, int hw_lds_words) {
  const size_t nc = (size_t)W * (K + 1);
  return 2 * 2 * 32 * 8 + 2 * 4 * 32 * 4 + 2 * 6 * 32 * 4 + 2 * 2 * 32 * 4 + 16 + nc * 8 + nc * 5 * 4 + (((size_t)V + 3) & ~(size_t)3) * 4 +
         (size_t)hw_lds_words * 4;
}
static inline size_t gam_beam_lds_bytes(int W, int K, int V, int hw_lds_words, bool lm = false) {
  const size_t base = gam_beam_lds_base(W, K, V, hw_lds_words);
  if (!lm) return base;
  return ((base + 15) & ~(size_t)15) + 2 * 32 * (8 + 16 + 3 * 4) + 2 * 32 * 4 + (((size_t)V + 3) & ~(size_t)3);
}

template <bool LM, bool NBEST = false>
__global__ __launch_bounds__(GAM_BEAM_NT) void gam_ctc_beam_kernel(GamBeamArgs a) {
  extern __shared__ uint4 gam_smem_beam[];
  unsigned char* p = reinterpret_cast<unsigned char*>(gam_smem_beam);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int Tp = a.Tp, V = a.V, W = a.W, K = a.K, blank = V - 1, K1 = K + 1;
  const int NC = W * K1;
  auto take = [&](size_t n) { unsigned char* r = p; p += n; return r; };
  unsigned long long* bh = reinterpret_cast<unsigned long long*>(take(2 * 32 * 8));    // [buf * 32 + i]
  unsigned long long* bph = reinterpret_cast<unsigned long long*>(take(2 * 32 * 8));
  float* bpb = reinterpret_cast<float*>(take(2 * 32 * 4));
  float* bpnb = reinterpret_cast<float*>(take(2 * 32 * 4));
  float* bacc = reinterpret_cast<float*>(take(2 * 32 * 4));
  float* bcb = reinterpret_cast<float*>(take(2 * 32 * 4));
  int* blen = reinterpret_cast<int*>(take(2 * 32 * 4));
  int* blast = reinterpret_cast<int*>(take(2 * 32 * 4));
  int* bnode = reinterpret_cast<int*>(take(2 * 32 * 4));
  int* bhn = reinterpret_cast<int*>(take(2 * 32 * 4));
  int* bpar = reinterpret_cast<int*>(take(2 * 32 * 4));
  int* bcm = reinterpret_cast<int*>(take(2 * 32 * 4));
  int* cid = reinterpret_cast<int*>(take(2 * 32 * 4));        // top-K ids of frame t at [(t & 1) * 32 + s]
  float* cval = reinterpret_cast<float*>(take(2 * 32 * 4));
  int* nbuf = reinterpret_cast<int*>(take(16));                // beam sizes [buf]
  unsigned long long* ckey = reinterpret_cast<unsigned long long*>(take((size_t)NC * 8));
  float* cpb = reinterpret_cast<float*>(take((size_t)NC * 4));
  float* cpnb = reinterpret_cast<float*>(take((size_t)NC * 4));
  float* cacc = reinterpret_cast<float*>(take((size_t)NC * 4));
  float* ccb = reinterpret_cast<float*>(take((size_t)NC * 4));
  int* chn = reinterpret_cast<int*>(take((size_t)NC * 4));
  float* row = reinterpret_cast<float*>(take((((size_t)V + 3) & ~(size_t)3) * 4));
  int* hw_sh = reinterpret_cast<int*>(p);
  // the LM's carve (gam_beam_lds_bytes): from the first 16-byte boundary after the hotword trie
  unsigned long long* bwh = nullptr;
  int4* bctx = nullptr;
  float *blm = nullptr, *bdl = nullptr;
  int *bcw = nullptr, *ccls = nullptr;
  signed char* cls_sh = nullptr;
  if constexpr (LM) {
    p = reinterpret_cast<unsigned char*>(gam_smem_beam) +
        ((gam_beam_lds_base(W, K, V, a.hw.trie != nullptr && a.hw.lds ? a.hw.words : 0) + 15) & ~(size_t)15);
    bwh = reinterpret_cast<unsigned long long*>(take(2 * 32 * 8));
    bctx = reinterpret_cast<int4*>(take(2 * 32 * 16));
    blm = reinterpret_cast<float*>(take(2 * 32 * 4));
    bdl = reinterpret_cast<float*>(take(2 * 32 * 4));
    bcw = reinterpret_cast<int*>(take(2 * 32 * 4));
    ccls = reinterpret_cast<int*>(take(2 * 32 * 4));       // classes of the top-K ids, beside cid
    cls_sh = reinterpret_cast<signed char*>(p);
  }

  int T = a.enc_len[b];
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
  const int* hw = a.hw.trie;
  if (hw != nullptr && a.hw.lds) {
    for (int i = tid; i < a.hw.words; i += GAM_BEAM_NT) hw_sh[i] = a.hw.trie[i];
    hw = hw_sh;
  }
  if (tid == 0) {       // the empty prefix: p_b = 0, p_nb = -inf, hotword state (root, 0)
    bh[0] = bph[0] = 0ull;
    bpb[0] = 0.f; bpnb[0] = -INFINITY; bacc[0] = 0.f; bcb[0] = 0.f;
    blen[0] = 0; blast[0] = -1; bnode[0] = -1; bhn[0] = 0; bpar[0] = -1; bcm[0] = 0;
    nbuf[0] = 1;
    if constexpr (LM) {   // an empty partial word, the state <s>, lm 0
      bwh[0] = 0ull;
      bctx[0] = make_int4(a.lm.lm_m > 0 ? a.lm.lm_bos : -1, -1, -1, -1);
      blm[0] = 0.f; bdl[0] = 0.f; bcw[0] = -1;
    }
  }

  const float* lpb = a.lp + (size_t)b * Tp * V;
  const int nrv = (V + 63) >> 6;
  float nxt[GAM_BEAM_RPL];       // wave 1: the row of the frame after the one whose top K it takes next
  // wave 1: the top K of the row in `x` (frame f) into cid / cval [(f & 1)], the row into LDS
  auto topk = [&](const float (&x)[GAM_BEAM_RPL], int f) {
    unsigned long long k[GAM_BEAM_RPL];
#pragma unroll
    for (int r = 0; r < GAM_BEAM_RPL; ++r) {
      const int v = lane + 64 * r;
      k[r] = (r < nrv && v < V - 1) ? (((unsigned long long)gam_beam_ord(x[r]) << 32) | (unsigned)(0xffff - v)) : 0ull;
      if (r < nrv && v < V) row[v] = x[r];
    }
    unsigned long long out;
    gam_beam_wave_topn(k, nrv, K, lane, out);
    if (lane < K) {
      cid[(f & 1) * 32 + lane] = 0xffff - (int)(out & 0xffff);
      cval[(f & 1) * 32 + lane] = gam_beam_unord((unsigned)(out >> 32));
      if constexpr (LM) ccls[(f & 1) * 32 + lane] = cls_sh[min(0xffff - (int)(out & 0xffff), V - 1)];
    }
  };
  if (wave == 1) {
    if constexpr (LM)     // (wave 1 alone reads the class table: its own LDS writes are ordered before its reads)
      for (int v = lane; v < V; v += 64) cls_sh[v] = (signed char)a.lm.lm_cls[v];
    float x[GAM_BEAM_RPL];
#pragma unroll
    for (int r = 0; r < GAM_BEAM_RPL; ++r) {
      const int v = min(lane + 64 * r, V - 1);
      if (r < nrv) x[r] = lpb[v];
    }
    const int t1 = T > 1 ? 1 : 0;
#pragma unroll
    for (int r = 0; r < GAM_BEAM_RPL; ++r) {
      const int v = min(lane + 64 * r, V - 1);
      if (r < nrv) nxt[r] = lpb[(size_t)t1 * V + v];
    }
    topk(x, 0);
  }
  __syncthreads();

  double off = 0.0;                  // wave 0: what the renormalisations subtracted so far
  int ncount = 0;                    // wave 0: prefix-trie nodes of this utterance so far
  int2* nodes = a.nodes + (size_t)b * Tp * W;
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1, nx = cur ^ 1;
    const int nb = nbuf[cur];
    const int N = nb * K1;
    const int* tk = cid + cur * 32;
    const float* tv = cval + cur * 32;
    // ---- phase 1: candidates
    for (int q = tid; q < N; q += GAM_BEAM_NT) {
      const int j = q / K1, s = q - j * K1;
      const int o = cur * 32 + j;
      const float pbj = bpb[o], pnbj = bpnb[o];
      const int lastj = blast[o], lenj = blen[o];
      const float tot = gam_beam_lse(pbj, pnbj);
      float pb, pnb, acc = bacc[o], cb = bcb[o];
      int hn = bhn[o], key;
      bool valid = true, reenter = false;
      if (s == K) {        // stay / repeat, and the extension of this entry's parent prefix by its last token
        pb = tot + row[blank];
        pnb = lenj > 0 ? pnbj + row[lastj] : -INFINITY;
        key = j * GAM_BEAM_KEY_STRIDE;
        const int par = bpar[o];
        if (par >= 0) {
          int sl = -1;
          for (int u = 0; u < K; ++u)
            if (tk[u] == lastj) sl = u;
          if (sl >= 0) {
            const int op = cur * 32 + par;
            const float pe = ((blen[op] > 0 && blast[op] == lastj) ? bpb[op] : gam_beam_lse(bpb[op], bpnb[op])) + tv[sl];
            reenter = pe > gam_beam_lse(pb, pnb);
            pnb = gam_beam_lse(pnb, pe);
            key = min(key, par * GAM_BEAM_KEY_STRIDE + lastj + 1);
          }
        }
      } else {
        const int c = tk[s];
        for (unsigned m = (unsigned)bcm[o]; m; m &= m - 1)     // merged into the entry that already is y_j + c
          if (blast[cur * 32 + __builtin_ctz(m)] == c) valid = false;
        pb = -INFINITY;
        pnb = ((lenj > 0 && c == lastj) ? pbj : tot) + tv[s];
        if (hw != nullptr) gam_beam_hw_step(hw, a.hw.nodes, a.hw.beta, c, hn, acc, cb);
        key = j * GAM_BEAM_KEY_STRIDE + c + 1;
      }
      float rank = gam_beam_lse(pb, pnb) + (cb + acc);
      if constexpr (LM) {   // the lm of the candidate's prefix: y_j's, plus d(y_j) when c completes y_j's partial word
        float lmv = blm[o];
        if (s != K && ccls[cur * 32 + s] != 0 && bwh[o] != 0ull) lmv += bdl[o];
        rank += lmv;
      }
      valid = valid && rank > -INFINITY;
      ckey[q] = valid ? gam_beam_key(gam_beam_ord(rank), key, q) : 0ull;
      cpb[q] = pb;
      cpnb[q] = pnb;
      cacc[q] = acc;
      ccb[q] = cb;
      chn[q] = hn << 1 | (reenter ? 1 : 0);
    }
    __syncthreads();
    if (wave == 0) {
      // ---- phase 2: the top W, then the new beam (lane i: entry i)
      unsigned long long k[GAM_BEAM_RPL];
      const int nr = (N + 63) >> 6;
#pragma unroll
      for (int r = 0; r < GAM_BEAM_RPL; ++r) {
        const int q = lane + 64 * r;
        k[r] = (r < nr && q < N) ? ckey[q] : 0ull;
      }
      unsigned long long sel;
      const int ns = gam_beam_wave_topn(k, nr, W, lane, sel);
      if (ns > 0) {
        float M = gam_beam_unord((unsigned)__builtin_amdgcn_readlane((int)(unsigned)(sel >> 32), 0));
        const bool act = lane < ns;
        const int q = act ? (int)(sel & 0xffff) : 0;
        const int j = q / K1, s = q - j * K1;
        const int o = cur * 32 + j;
        const bool ext = act && s != K;
        const int hnre = chn[q];
        const bool re = act && s == K && (hnre & 1);     // a stay whose merged extension outweighs it: its last token re-enters at t
        const unsigned long long hj = bh[o];
        const int c = ext ? tk[s] : blast[o];
        unsigned long long lwh = 0ull;
        int4 lcx = make_int4(-1, -1, -1, -1);
        float llm = 0.f, ldl = 0.f;
        int lcw = -1;
        if constexpr (LM) {   // the new entry's LM state; an extension whose partial word is non-empty queries d and its word id
          const unsigned long long whj = bwh[o];
          const int4 cj = bctx[o];
          const int cl = ext ? ccls[cur * 32 + s] : 0;
          const bool done = ext && cl != 0 && whj != 0ull;      // c completes y_j's partial word
          llm = done ? blm[o] + bdl[o] : blm[o];
          lcx = done ? make_int4(bcw[o], cj.x, cj.y, cj.z) : cj;
          lwh = !ext ? whj : (cl == 0 ? whj * GAM_BEAM_HASH_P + (unsigned long long)(c + 1) : (cl == 1 ? (unsigned long long)(c + 1) : 0ull));
          if (!ext) {
            ldl = bdl[o];
            lcw = bcw[o];
          } else if (lwh != 0ull) {
            ldl = a.lm.lm_alpha * gam_lm_query(a.lm, true, lwh, lcw, lcx) + a.lm.lm_beta;
          }
          M -= __int_as_float(__builtin_amdgcn_readlane(__float_as_int(llm), 0));     // (p_b / p_nb keep O(one frame))
        }
        off += (double)M;
        const unsigned long long h = ext ? hj * GAM_BEAM_HASH_P + (unsigned long long)(c + 1) : hj;
        const unsigned long long ph = ext ? hj : bph[o];
        const int len = blen[o] + (ext ? 1 : 0);
        int pnode = re ? bnode[cur * 32 + bpar[o]] : bnode[o];
        const unsigned long long em = __ballot(ext || re);
        if (ext || re) {
          const int idx = ncount + __popcll(em & ((1ull << lane) - 1));
          nodes[idx] = make_int2(pnode, (c << 13) | t);
          pnode = idx;
        }
        ncount += __popcll(em);
        int par = -1;
        for (int i = 0; i < ns; ++i) {
          const unsigned long long hi = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(h >> 32), i) << 32) |
                                        (unsigned)__builtin_amdgcn_readlane((int)(unsigned)h, i);
          const int li = __builtin_amdgcn_readlane(len, i);
          if (par < 0 && len > 0 && li == len - 1 && hi == ph) par = i;
        }
        int cm = 0;
        for (int i = 0; i < ns; ++i) {
          const unsigned long long bm = __ballot(act && par == i);
          if (lane == i) cm = (int)(unsigned)bm;
        }
        if (act) {
          const int d = nx * 32 + lane;
          bh[d] = h; bph[d] = ph;
          bpb[d] = cpb[q] - M; bpnb[d] = cpnb[q] - M; bacc[d] = cacc[q]; bcb[d] = ccb[q];
          blen[d] = len; blast[d] = c; bnode[d] = pnode; bhn[d] = hnre >> 1; bpar[d] = par; bcm[d] = cm;
          if constexpr (LM) {
            bwh[d] = lwh; bctx[d] = lcx; blm[d] = llm; bdl[d] = ldl; bcw[d] = lcw;
          }
        }
      }
      if (lane == 0) nbuf[nx] = ns;
    } else if (wave == 1 && t + 1 < T) {
      // ---- the top K of frame t + 1 (its row arrived during this frame); load the row of frame t + 2
      float x[GAM_BEAM_RPL];
#pragma unroll
      for (int r = 0; r < GAM_BEAM_RPL; ++r) x[r] = nxt[r];
      const int t2 = t + 2 < T ? t + 2 : T - 1;
#pragma unroll
      for (int r = 0; r < GAM_BEAM_RPL; ++r) {
        const int v = min(lane + 64 * r, V - 1);
        if (r < nrv) nxt[r] = lpb[(size_t)t2 * V + v];
      }
      topk(x, t + 1);
    }
    __syncthreads();
  }

  // ---- final pick (pending hotword bonus dropped) and backtrack
  if (wave == 0) {
    const int fb = T & 1;
    const int nb = nbuf[fb];
    const int d = fb * 32 + lane;
    const float lse = lane < nb ? gam_beam_lse(bpb[d], bpnb[d]) : -INFINITY;
    float val = lane < nb ? lse + bcb[d] : -INFINITY;
    float lmf = 0.f;
    if constexpr (LM) {   // complete the last partial word, then </s>
      if (lane < nb) {
        int4 cx = bctx[d];
        lmf = blm[d];
        if (bwh[d] != 0ull) {
          lmf += bdl[d];
          cx = make_int4(bcw[d], cx.x, cx.y, cx.z);
        }
        int w = a.lm.lm_eos;
        lmf += a.lm.lm_alpha * gam_lm_query(a.lm, false, 0ull, w, cx);
        val += lmf;
      }
    }
    if constexpr (NBEST) {   // the nb.n best entries instead of the best one (gam_search.h): the same value, key and arithmetic
      const double lp_ = (double)lse + off;
      const float sc = lane < nb ? (LM ? (float)(lp_ + (double)bcb[d] + (double)lmf) : (float)(lp_ + (double)bcb[d])) : -INFINITY;
      gam_beam_emit_nbest(a.nb, b, Tp, lane < nb, val, sc, (float)lp_, lane < nb ? blen[d] : 0, lane < nb ? bnode[d] : -1, nodes, a.ids,
                          a.frames, a.counts, a.score, a.logp, lane);
      return;
    }
    const unsigned long long key = lane < nb ? (((unsigned long long)gam_beam_ord(val) << 32) | (unsigned)(0xffff - lane)) : 0ull;
    const unsigned long long m = gam_beam_wave_max(key);
    const int best = m ? 0xffff - (int)(m & 0xffff) : -1;
    if (best < 0) {
      if (lane == 0) {
        a.counts[b] = 0;
        a.score[b] = -INFINITY;
        a.logp[b] = -INFINITY;
      }
    } else if (lane == best) {
      const double lp_ = (double)lse + off;
      a.logp[b] = (float)lp_;
      a.score[b] = LM ? (float)(lp_ + (double)bcb[d] + (double)lmf) : (float)(lp_ + (double)bcb[d]);
      const int n = blen[d];
      a.counts[b] = n;
      int* ids = a.ids + (size_t)b * Tp;
      int* fr = a.frames + (size_t)b * Tp;
      int node = bnode[d];
      for (int i = n - 1; i >= 0; --i) {
        const int2 e = nodes[node];
        ids[i] = e.y >> 13;
        fr[i] = e.y & 8191;
        node = e.x;
      }
    }
  }
}
