// gam_beam_stream.h -- gam_beam.h's CTC prefix beam search for ONE stream of any length fed in pieces (gam_op_ctc_beam_stream).
//
// The contract is gam_beam.h's, unchanged: the candidates, the merge and re-entry rule, the origin-key tie rule, hotwords and LM per
// gam_search.h, the per-frame renormalisation into `off`, two barriers per frame with wave 1 preparing the top K of the next row.  The
// frame loop below is the batch kernel's text with three differences: rows are addressed by the call's local index i while every frame
// written to a node is the stream frame t_base + i; a node is {parent, token, frame, 0} (a 31-bit frame does not fit beside parent and
// token in 64 bits); and the rebase below.  The loop is NOT shared with gam_ctc_beam_kernel through functions: the batch kernel's four
// instantiations keep their text and with it their compiler numbers, and tests/test_hip_ctc_beam_stream.py holds
// the two together bit for bit.
//
// A call: load the state (BEGIN: the empty prefix, with an LM the state <s>), the top K of local row 0 in the prologue, rows 0 .. n - 1
// as stream frames t_base .. t_base + n - 1, store the state.  Nothing is stored to the state inside the frame loop.  END: the final
// pick (pending hotword bonus dropped, last word and </s> added) and the backtrack behind the call's last row.  n = 0 is legal with
// either flag, both or none.  A stream that ends without a frame gives count 0, score = logp = 0, as the batch kernel's T = 0.
//
// Rebase: p_b / p_nb stay O(one frame) (gam_beam.h), but an entry's committed hotword bonus and its LM term are plain fp32 sums that
// reach 10^4 over an hour, where an fp32 ulp exceeds the rank differences the search decides on.  At every stream frame t > 0 that is a
// multiple of GAM_BEAM_STREAM_REBASE the best new entry's committed bonus and LM term are subtracted from every new entry's and added
// to two fp64 offsets of the state; `score` adds them back in fp64.  Every rank moves by the same amount, so the order stands; the
// next frame's renormalisation moves p_b / p_nb (and `off`) by the opposite amount, so logp stands.  The rebase frames are stream
// frames: no cutting moves them, and a stream of at most GAM_BEAM_STREAM_REBASE frames is the batch kernel's arithmetic throughout.
//
// State record (caller-owned, gam_ctc_beam_stream_bytes): GamBeamStreamHdr | 32 x GamBeamStreamEntry (the beam, saved as buffer 0) |
// the node pool int4 [max_frames x W] (at most W nodes per frame, as in gam_beam.h).
// Refusals (status[0] = 0, nothing else written): the state is not begun or has ended; t_base is not the state's next frame; W or V is
// not what BEGIN saw; the hotword or LM generation has moved (gam_handle::hw_gen / lm_gen); t_base + n > max_frames.  An accepted call
// writes status[0] = 1.
#pragma once
#include "gam_beam.h"

#define GAM_BEAM_STREAM_REBASE 1024       // a power of two, <= 8192
#define GAM_BEAM_F_BEGIN 1                // include/gigaam_hip.h GAM_BEAM_STREAM_BEGIN / _END
#define GAM_BEAM_F_END 2
#define GAM_BEAM_ST_BEGUN 0x6265616d      // phase words; anything else, zeros included, is "not begun"
#define GAM_BEAM_ST_ENDED 0x656e6465

struct GamBeamStreamHdr {
  int phase, W, V, hw_gen, lm_gen;
  int nb, ncount;                 // beam size, prefix-trie nodes so far
  int next, max_frames, t0;       // the next stream frame, the pool's frames, the frame BEGIN started at
  int pad0[2];
  double off, cb_off, lm_off;     // what the renormalisations / the rebases of the committed bonus / of the LM term subtracted so far
  int pad1[14];
};
struct GamBeamStreamEntry {       // gam_beam.h's LDS beam state of one entry; the LM fields are written by the <true> kernel only
  unsigned long long h, ph;
  float pb, pnb, acc, cb;
  int len, last, node, hn, par, cm;
  unsigned long long wh;
  int4 ctx;
  float lm, dl;
  int cw, pad;
};
static_assert(sizeof(GamBeamStreamHdr) == 128 && offsetof(GamBeamStreamHdr, off) == 48 && sizeof(GamBeamStreamEntry) == 96,
              "beam stream state layout");
#define GAM_BEAM_STREAM_HDR_BYTES (sizeof(GamBeamStreamHdr) + 32 * sizeof(GamBeamStreamEntry))      // 3200: the node pool starts here

struct GamBeamStreamArgs {
  const float* lp;       // [n, V] log-probs of this call
  int n, t_base, max_frames, flags;     // max_frames: what the caller's state_bytes hold for this W
  int V, W, K;
  int hw_gen, lm_gen;
  GamHwArgs hw;
  GamLmArgs lm;
  void* state;
  int* ids;              // [max_frames]   (END only, as count / score / logp)
  int* frames;           // [max_frames]
  int* count;            // [1]
  double* score;         // [1]
  double* logp;          // [1]
  int* status;           // [1]
};

template <bool LM>
__global__ __launch_bounds__(GAM_BEAM_NT) void gam_ctc_beam_stream_kernel(GamBeamStreamArgs a) {
  extern __shared__ uint4 gam_smem_beam_stream[];
  unsigned char* p = reinterpret_cast<unsigned char*>(gam_smem_beam_stream);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n, V = a.V, W = a.W, K = a.K, blank = V - 1, K1 = K + 1;
  const int NC = W * K1;
  GamBeamStreamHdr* hdr = static_cast<GamBeamStreamHdr*>(a.state);
  GamBeamStreamEntry* ent = reinterpret_cast<GamBeamStreamEntry*>(hdr + 1);
  int4* nodes = reinterpret_cast<int4*>(ent + 32);

  // ---- the call against the state (every thread reads the header before the first barrier; it is written behind the last)
  const bool begin = (a.flags & GAM_BEAM_F_BEGIN) != 0;
  int maxf = a.max_frames, t0 = a.t_base, nb0 = 1, ncount = 0;
  double off = 0.0, cb_off = 0.0, lm_off = 0.0;
  bool ok = true;
  if (!begin) {
    ok = hdr->phase == GAM_BEAM_ST_BEGUN && hdr->next == a.t_base && hdr->W == W && hdr->V == V && hdr->hw_gen == a.hw_gen &&
         hdr->lm_gen == a.lm_gen && hdr->max_frames <= a.max_frames && hdr->nb >= 0 && hdr->nb <= W;
    if (ok) {
      maxf = hdr->max_frames; t0 = hdr->t0; nb0 = hdr->nb; ncount = hdr->ncount;
      off = hdr->off; cb_off = hdr->cb_off; lm_off = hdr->lm_off;
    }
  }
  ok = ok && (long long)a.t_base + n <= (long long)maxf;
  if (!ok) {
    if (tid == 0) a.status[0] = 0;
    return;
  }

  auto take = [&](size_t nbytes) { unsigned char* r = p; p += nbytes; return r; };
  unsigned long long* bh = reinterpret_cast<unsigned long long*>(take(2 * 32 * 8));    // [buf * 32 + i]   (the carve of gam_beam.h)
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
  int* cid = reinterpret_cast<int*>(take(2 * 32 * 4));        // top-K ids of local row i at [(i & 1) * 32 + s]
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
  unsigned long long* bwh = nullptr;
  int4* bctx = nullptr;
  float *blm = nullptr, *bdl = nullptr;
  int *bcw = nullptr, *ccls = nullptr;
  signed char* cls_sh = nullptr;
  if constexpr (LM) {
    p = reinterpret_cast<unsigned char*>(gam_smem_beam_stream) +
        ((gam_beam_lds_base(W, K, V, a.hw.trie != nullptr && a.hw.lds ? a.hw.words : 0) + 15) & ~(size_t)15);
    bwh = reinterpret_cast<unsigned long long*>(take(2 * 32 * 8));
    bctx = reinterpret_cast<int4*>(take(2 * 32 * 16));
    blm = reinterpret_cast<float*>(take(2 * 32 * 4));
    bdl = reinterpret_cast<float*>(take(2 * 32 * 4));
    bcw = reinterpret_cast<int*>(take(2 * 32 * 4));
    ccls = reinterpret_cast<int*>(take(2 * 32 * 4));
    cls_sh = reinterpret_cast<signed char*>(p);
  }

  const int* hw = a.hw.trie;
  if (hw != nullptr && a.hw.lds) {
    for (int i = tid; i < a.hw.words; i += GAM_BEAM_NT) hw_sh[i] = a.hw.trie[i];
    hw = hw_sh;
  }
  // ---- the beam into buffer 0: the empty prefix (BEGIN), else the state's
  if (begin) {
    if (tid == 0) {
      bh[0] = bph[0] = 0ull;
      bpb[0] = 0.f; bpnb[0] = -INFINITY; bacc[0] = 0.f; bcb[0] = 0.f;
      blen[0] = 0; blast[0] = -1; bnode[0] = -1; bhn[0] = 0; bpar[0] = -1; bcm[0] = 0;
      nbuf[0] = 1;
      if constexpr (LM) {
        bwh[0] = 0ull;
        bctx[0] = make_int4(a.lm.lm_m > 0 ? a.lm.lm_bos : -1, -1, -1, -1);
        blm[0] = 0.f; bdl[0] = 0.f; bcw[0] = -1;
      }
    }
  } else if (wave == 0) {
    if (lane < nb0) {
      const GamBeamStreamEntry& e = ent[lane];
      bh[lane] = e.h; bph[lane] = e.ph;
      bpb[lane] = e.pb; bpnb[lane] = e.pnb; bacc[lane] = e.acc; bcb[lane] = e.cb;
      blen[lane] = e.len; blast[lane] = e.last; bnode[lane] = e.node; bhn[lane] = e.hn; bpar[lane] = e.par; bcm[lane] = e.cm;
      if constexpr (LM) {
        bwh[lane] = e.wh; bctx[lane] = e.ctx; blm[lane] = e.lm; bdl[lane] = e.dl; bcw[lane] = e.cw;
      }
    }
    if (lane == 0) nbuf[0] = nb0;
  }

  const float* lpb = a.lp;
  const int nrv = (V + 63) >> 6;
  float nxt[GAM_BEAM_RPL];       // wave 1: the row after the one whose top K it takes next
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
  if (wave == 1 && n > 0) {
    if constexpr (LM)     // (wave 1 alone reads the class table: its own LDS writes are ordered before its reads)
      for (int v = lane; v < V; v += 64) cls_sh[v] = (signed char)a.lm.lm_cls[v];
    float x[GAM_BEAM_RPL];
#pragma unroll
    for (int r = 0; r < GAM_BEAM_RPL; ++r) {
      const int v = min(lane + 64 * r, V - 1);
      if (r < nrv) x[r] = lpb[v];
    }
    const int i1 = n > 1 ? 1 : 0;
#pragma unroll
    for (int r = 0; r < GAM_BEAM_RPL; ++r) {
      const int v = min(lane + 64 * r, V - 1);
      if (r < nrv) nxt[r] = lpb[(size_t)i1 * V + v];
    }
    topk(x, 0);
  }
  __syncthreads();

  for (int i = 0; i < n; ++i) {
    const int t = a.t_base + i;        // the stream frame: what a node records, what the rebase goes by
    const int cur = i & 1, nx = cur ^ 1;
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
      if constexpr (LM) {
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
        if constexpr (LM) {
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
        float ncb = ccb[q];
        if (t > 0 && (t & (GAM_BEAM_STREAM_REBASE - 1)) == 0) {      // the rebase: the best entry's sums leave every entry's
          const float cb0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ncb), 0));
          ncb -= cb0;
          cb_off += (double)cb0;
          if constexpr (LM) {
            const float lm0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(llm), 0));
            llm -= lm0;
            lm_off += (double)lm0;
          }
        }
        const unsigned long long h = ext ? hj * GAM_BEAM_HASH_P + (unsigned long long)(c + 1) : hj;
        const unsigned long long ph = ext ? hj : bph[o];
        const int len = blen[o] + (ext ? 1 : 0);
        int pnode = re ? bnode[cur * 32 + bpar[o]] : bnode[o];
        const unsigned long long em = __ballot(ext || re);
        if (ext || re) {
          const int idx = ncount + __popcll(em & ((1ull << lane) - 1));
          nodes[idx] = make_int4(pnode, c, t, 0);
          pnode = idx;
        }
        ncount += __popcll(em);
        int par = -1;
        for (int u = 0; u < ns; ++u) {
          const unsigned long long hi = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(h >> 32), u) << 32) |
                                        (unsigned)__builtin_amdgcn_readlane((int)(unsigned)h, u);
          const int li = __builtin_amdgcn_readlane(len, u);
          if (par < 0 && len > 0 && li == len - 1 && hi == ph) par = u;
        }
        int cm = 0;
        for (int u = 0; u < ns; ++u) {
          const unsigned long long bm = __ballot(act && par == u);
          if (lane == u) cm = (int)(unsigned)bm;
        }
        if (act) {
          const int d = nx * 32 + lane;
          bh[d] = h; bph[d] = ph;
          bpb[d] = cpb[q] - M; bpnb[d] = cpnb[q] - M; bacc[d] = cacc[q]; bcb[d] = ncb;
          blen[d] = len; blast[d] = c; bnode[d] = pnode; bhn[d] = hnre >> 1; bpar[d] = par; bcm[d] = cm;
          if constexpr (LM) {
            bwh[d] = lwh; bctx[d] = lcx; blm[d] = llm; bdl[d] = ldl; bcw[d] = lcw;
          }
        }
      }
      if (lane == 0) nbuf[nx] = ns;
    } else if (wave == 1 && i + 1 < n) {
      // ---- the top K of row i + 1 (it arrived during this frame); load row i + 2
      float x[GAM_BEAM_RPL];
#pragma unroll
      for (int r = 0; r < GAM_BEAM_RPL; ++r) x[r] = nxt[r];
      const int i2 = i + 2 < n ? i + 2 : n - 1;
#pragma unroll
      for (int r = 0; r < GAM_BEAM_RPL; ++r) {
        const int v = min(lane + 64 * r, V - 1);
        if (r < nrv) nxt[r] = lpb[(size_t)i2 * V + v];
      }
      topk(x, i + 1);
    }
    __syncthreads();
  }

  if (wave != 0) return;
  const bool end = (a.flags & GAM_BEAM_F_END) != 0;
  const int fb = n & 1;
  const int nb = nbuf[fb];
  const int d = fb * 32 + lane;
  // ---- store the state: the beam as buffer 0, then the header
  if (lane < nb) {
    GamBeamStreamEntry& e = ent[lane];
    e.h = bh[d]; e.ph = bph[d];
    e.pb = bpb[d]; e.pnb = bpnb[d]; e.acc = bacc[d]; e.cb = bcb[d];
    e.len = blen[d]; e.last = blast[d]; e.node = bnode[d]; e.hn = bhn[d]; e.par = bpar[d]; e.cm = bcm[d];
    if constexpr (LM) {
      e.wh = bwh[d]; e.ctx = bctx[d]; e.lm = blm[d]; e.dl = bdl[d]; e.cw = bcw[d];
    }
  }
  if (lane == 0) {
    hdr->phase = end ? GAM_BEAM_ST_ENDED : GAM_BEAM_ST_BEGUN;
    hdr->W = W; hdr->V = V; hdr->hw_gen = a.hw_gen; hdr->lm_gen = a.lm_gen;
    hdr->nb = nb; hdr->ncount = ncount;
    hdr->next = a.t_base + n; hdr->max_frames = maxf; hdr->t0 = t0;
    hdr->off = off; hdr->cb_off = cb_off; hdr->lm_off = lm_off;
    a.status[0] = 1;
  }
  if (!end) return;

  // ---- final pick (pending hotword bonus dropped) and backtrack
  if (a.t_base + n == t0) {      // a stream without a frame
    if (lane == 0) {
      a.count[0] = 0;
      a.score[0] = 0.0;
      a.logp[0] = 0.0;
    }
    return;
  }
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
  const unsigned long long key = lane < nb ? (((unsigned long long)gam_beam_ord(val) << 32) | (unsigned)(0xffff - lane)) : 0ull;
  const unsigned long long m = gam_beam_wave_max(key);
  const int best = m ? 0xffff - (int)(m & 0xffff) : -1;
  if (best < 0) {
    if (lane == 0) {
      a.count[0] = 0;
      a.score[0] = -INFINITY;
      a.logp[0] = -INFINITY;
    }
  } else if (lane == best) {
    const double lp_ = (double)lse + off;
    a.logp[0] = lp_;
    a.score[0] = (LM ? lp_ + (double)bcb[d] + (double)lmf : lp_ + (double)bcb[d]) + cb_off + lm_off;
    const int cnt = blen[d];
    a.count[0] = cnt;
    int node = bnode[d];
    for (int i = cnt - 1; i >= 0; --i) {
      const int4 e = nodes[node];
      a.ids[i] = e.y;
      a.frames[i] = e.z;
      node = e.x;
    }
  }
}
