// gam_api.hip -- host side of libgigaam_hip.so: handle, weight re-layout, workspace,
// per-batch orchestration of the gfx950 kernels, and the extern "C" boundary declared in
// include/gigaam_hip.h.  One call per batch; nothing here synchronises the host except
// workspace growth.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/gigaam_hip.h"
#include "gam_align.h"
#include "gam_align_long.h"
#include "gam_kws.h"
#include "gam_attn.h"
#include "gam_beam.h"
#include "gam_beam_stream.h"
#include "gam_rnnt_beam.h"
#include "gam_rnnt_beam_stream.h"
#include "gam_attn16.h"
#include "gam_comm.h"
#include "gam_common.h"
#include "gam_convmod.h"
#include "gam_decode.h"
#include "gam_rnnt_stream.h"
#include "gam_rnnt_align.h"
#include "gam_confidence.h"
#include "gam_decode_cluster.h"
#include "gam_frontend.h"
#include "gam_gemm.h"
#include "gam_gemm_sp.h"
#include "gam_norm.h"
#include "gam_pack.h"
#include "gam_resample.h"
#include "gam_stem.h"
#include "gam_stitch.h"

namespace {

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
  int64_t numel() const {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    return n;
  }
};

// One device allocation.  It frees itself and cannot be copied: whatever the handle holds as a DevBuf, or in a container of them, goes
// with `delete h` (DESIGN.md "Handle memory").
struct DevBuf {
  float* p = nullptr;
  size_t cap = 0;  // floats
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }   // (o frees what this held)
  ~DevBuf() { (void)release(); }
  hipError_t release() {
    const hipError_t e = p ? hipFree(p) : hipSuccess;
    p = nullptr; cap = 0;
    return e;
  }
  // The one way a buffer gets memory: what it held is freed first, its contents are not kept.
  hipError_t alloc(size_t floats) {
    hipError_t e = release();
    if (e == hipSuccess) e = hipMalloc(&p, floats * sizeof(float));
    if (e == hipSuccess) cap = floats; else p = nullptr;
    return e;
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }   // the typed view of a buffer of ints / table slots
};

struct W16 {            // split-fp16 operand of one weight matrix (gam_gemm_sp.h): W * 2^s = hi + lo
  _Float16* sp = nullptr;   // (hi, lo) in the sp32 layout
  _Float16* h16 = nullptr;  // GAM_GEMM_F16: the hi plane as the one-term kernel walks it (row-major; a tap-permuted copy for the stem conv)
  float inv = 1.0f;         // 2^-s
};

struct LayerW {
  float *ln_ff1_w, *ln_ff1_b, *ff1_w1, *ff1_b1, *ff1_w2, *ff1_b2;
  float *ln_att_w, *ln_att_b, *wqkv, *bqkv, *wo, *bo;   // rows [W_q; W_k; W_v]
  float *wpos, *pos_u, *pos_v;  // rel_pos only
  float *ln_conv_w, *ln_conv_b, *pw1_w, *pw1_b, *dw_w, *dw_b, *cn_scale, *cn_shift, *pw2_w, *pw2_b;
  float *ln_ff2_w, *ln_ff2_b, *ff2_w1, *ff2_b1, *ff2_w2, *ff2_b2;
  float *ln_out_w, *ln_out_b;
  W16 s_ff1_w1, s_ff1_w2, s_wqkv, s_wo, s_wpos, s_pw1, s_pw2, s_ff2_w1, s_ff2_w2;
};

struct ProfEvent {
  hipEvent_t a, b;
  int cls;
};

}  // namespace

struct gam_handle {
  gam_config cfg;
  int device = 0;
  bool finalized = false;
  bool has_encoder = false, has_head = false;
  std::map<std::string, HostTensor> staged;
  std::vector<DevBuf> owned;   // every weight and table of gam_finalize (dev_upload); the float* / W16 members below are views into it
  std::string err;

  // frontend
  float* dft_basis = nullptr;
  int* mel_band = nullptr;   // [3 * n_mels] per mel band: first / one-past-last bin with a non-zero weight, offset into mel_wts
  float* mel_wts = nullptr;  // the non-zero stretch of every band's filter, band after band (gam_powmel_kernel keeps it in LDS)
  int mel_nw = 0;            // floats in mel_wts
  int nf = 0, kpad = 0;
  // stem
  float *c1_w = nullptr, *c1_b = nullptr, *c2_w = nullptr, *c2_b = nullptr, *lin_w = nullptr, *lin_b = nullptr;
  W16 s_c1, s_c2, s_lin;
  int gemm_mode = 1;  // GAM_GEMM_F16X3
  int f1 = 0, f2 = 0;  // conv2d: feature bins after stage 1 / 2
  // layers
  std::vector<LayerW> layers;
  float *rot_cos = nullptr, *rot_sin = nullptr;
  float* rel_pe = nullptr;  // rel_pos: sinusoid table, row r + (max_len-1) <-> relative position r
  float* rel_pe_sp = nullptr;   // the same table in the sp32 layout (same bytes, same row offsets): linear_pos's split-fp16 A operand
  // heads
  float *ctc_w = nullptr, *ctc_b = nullptr;
  float *emo_w = nullptr, *emo_b = nullptr;
  float *jn_enc_w = nullptr, *jn_enc_b = nullptr, *jn_pred_t = nullptr, *jn_pred_b = nullptr;
  float *jn_out_w = nullptr, *jn_out_b = nullptr, *lstm_whh_t = nullptr, *lstm_tab = nullptr;
  float *lstm_whh_q = nullptr, *jn_pred_q = nullptr;   // [k/4][row][4] re-layouts for the cluster decode kernel
  float* jn_pred_w = nullptr;   // W_pred as uploaded ([JH, PH] row-major): the GEMM form of gam_rnnt_joint
  DevBuf jz, jp, jl;            // gam_rnnt_joint workspace: hidden layer, predictor projection, logits
  float *lstm_wih_x = nullptr, *lstm_whh_x = nullptr, *lstm_bias_x = nullptr;   // predictor layers above the first (gam_decode.h)
  int use_rowscale = 1;         // GAM_ROWSCALE=0: no per-row pre-scale of the LayerNorm-produced GEMM operands (A/B switch)
  int use_range = 1;            // GAM_RANGE=0: no range guard on the unscaled operands (A/B switch)
  int ncu = 256;                // compute units of the device (hipDeviceAttributeMultiprocessorCount)
  int rnnt_cluster = -1;        // GAM_RNNT_CLUSTER: 0 = one workgroup per utterance, N = force N per utterance, -1 = auto
  int rnnt_coop = 1;            // GAM_RNNT_COOP=0: plain instead of cooperative launch of the cluster kernel
  int rnnt_force_timeout = 0;   // GAM_RNNT_FORCE_TIMEOUT=1 (test hook): odd utterances' clusters report a failed hand-off
  int rnnt_no_repair = 0;       // GAM_RNNT_NO_REPAIR=1 (test hook): no repair pass behind the cluster kernel
  int rnnt_exclusive = 0;       // GAM_RNNT_EXCLUSIVE=1: decode workgroups ask for their CU's whole LDS, so nothing that uses LDS is placed beside them
                                // (r05's protection; not needed since r06 removed the packed-fp32 instructions that a neighbour's MFMAs disturbed --
                                // tests/test_hip_hardening.py runs the decode beside another stream's GEMM both ways)
  int last_rnnt_c = 0, last_rnnt_kern = -1, last_rnnt_refused = 0;   // what the last gam_rnnt_greedy launched (gam_rnnt_last_decode)
  DevBuf rnnt_x;                // hand-off granules + status word of the cluster kernel
  // The decode class owns ONE set of scratch per handle (tok / logits / encp / rnnt_x / jz / jp / jl / dec_splitk_ws).  Every decode-class
  // entry point records dec_evt behind its last launch; a decode-class call on ANOTHER stream waits for it first (DecodeScope), so two
  // decodes of one handle are ordered whatever streams the caller puts them on (an overlapped decode on the side stream followed
  // by a serial one on the launch stream overwrote the scratch the first was still reading).
  hipEvent_t dec_evt = nullptr;
  hipStream_t dec_stream = nullptr;
  bool dec_evt_set = false;

  // workspace (grow-only)
  DevBuf wavp, spec, img, c2, xin, y1, x, y, yr, hbuf, qkv, ctx, ubuf, zbuf, tok, logits, encp, pbuf, aplanes;
  DevBuf op_planes, op_sp, splitk_ws;   // gam_op_gemm operand planes; split-K partial sums
  DevBuf align_star;                    // wildcard emissions of gam_ctc_align_star, B x T' floats (gam_ctc_star_row_kernel)
  DevBuf align_bp;                      // CTC alignment backpointers when they do not fit the kernel's LDS (gam_align.h)
  DevBuf align_long_ws;                 // long-utterance CTC alignment (gam_align_long.h): backpointers | edges | rows | offsets | path | ctrl
  DevBuf greedy_long_ws;                // long-utterance CTC greedy decode (gam_stitch.h): labels [T] | block counts -> offsets, as ints
  size_t al_ws_limit = GAM_AL_WS_DEFAULT;   // bytes that workspace may take (gam_set_ctc_align_workspace; GAM_CTC_ALIGN_WS at gam_create)
  DevBuf beam_nodes;                    // CTC beam search prefix-trie nodes, B x T' x W (gam_beam.h)
  DevBuf rb_ws, rb_nodes;               // RNN-T beam search: predictor-state slots + logit rows, prefix-trie nodes (gam_rnnt_beam.h)
  DevBuf ra_g, ra_pp, ra_lat, ra_bp;    // transducer alignment (gam_rnnt_align.h): predictor outputs, their projection, the (lb, le)
                                        // lattice of one slice, backpointers that do not fit the sweep kernel's LDS
  DevBuf cf_stats;                      // token confidence (gam_confidence.h): the CTC pass's per-frame (argmax, measure), B x T' x 8 bytes
  size_t ra_ws_limit = GAM_RA_WS_DEFAULT;   // bytes of lattice per slice (gam_set_rnnt_align_workspace; GAM_RNNT_ALIGN_WS at gam_create)
  DevBuf hw_trie;                       // hotword trie of gam_set_hotwords (CSR, gam_search.h), ints: offsets | edges; empty = no hotwords
  int hw_nodes = 0, hw_words = 0, hw_max_tok = -1;
  float hw_boost = 0.f;
  int hw_gen = 0, lm_gen = 0;           // count the successful gam_set_hotwords / gam_set_lm calls, as kw_gen: a beam stream state remembers both
  // the keyword set of gam_set_keywords (gam_kws.h): offsets [K + 1] | tokens | min_score [K] (f32 bits) in one buffer of ints; empty = no set
  DevBuf kw_dev;
  int kw_K = 0, kw_ntok = 0, kw_max_tok = -1;
  int kw_gen = 0;                       // counts the successful gam_set_keywords calls (an identical set counts too): a stream state remembers the one it began under
  DevBuf kws_mb;                        // keyword search: per row {maximum, blank's emission}, B x T' x 8 bytes
  // the n-gram LM of gam_set_lm (gam_search.h): token classes [lm_V], word / n-gram table slots (uint4); lm_ng empty = no LM
  DevBuf lm_cls, lm_wt, lm_ng;
  int lm_V = 0, lm_wslots = 0, lm_wprobe = 0, lm_nslots = 0, lm_nprobe = 0, lm_order = 0, lm_bos = 0, lm_eos = 0, lm_unk = 0;
  float lm_unk_logp = 0.f, lm_alpha = 0.f, lm_beta = 0.f;
  DevBuf dec_splitk_ws;                 // split-K partial sums of the DECODE class's GEMMs: a decode may run on a side stream beside
                                        // the next batch's encoder (r05), so it shares no scratch with it (tok / logits / encp / rnnt_x
                                        // are the decode's alone already)
  int last_rows = 0, last_rows_padded = 0;   // token rows the layers of the last gam_encode* call ran on / would run on padded (gam_last_encode_rows)
  DevBuf pack_idx;      // packed rows (gam_pack.h): cu [B + 1] | row_t [rows] | row_src [rows], as ints
  int use_pack = 1;     // GAM_PACK=0: ragged batches keep the padded row layout even when the caller gave host lengths (A/B switch); 2: packed
                        // rows also below graph_max_rows token rows (tests: the small cases)
  int use_splitk = 1;   // GAM_SPLITK=0 disables split-K for small grids
  int fuse_reduce = 1;  // GAM_FUSE_REDUCE=0: the split-K reduce of a residual GEMM stays a kernel of its own (A/B switch)
  // hipGraph replay of the Conformer-layer launch sequence for small batches (launch-bound: a 5 s clip is
  // ~450 launches of 5-25 us).  Keyed on the shape; captured the second time a shape is seen (the first
  // call sizes every workspace and sets the kernel attributes); dropped whenever a workspace buffer moves.
  int use_graph = 1;            // GAM_GRAPH=0 disables
  int graph_max_rows = 2048;    // only below the large-batch (sp32) regime
  uint64_t ws_generation = 0;   // bumped by every workspace (re)allocation
  struct GraphEntry {
    enum Seen { UNSEEN, SEEN_ONCE, PLAIN_ONLY };   // first sight: plain launches; second: capture; PLAIN_ONLY: capture refused or cache full
    uint64_t gen = 0; Seen seen = UNSEEN; hipGraphExec_t exec = nullptr;   // (exec set: replayed from the third sight on)
  };
  std::map<std::vector<int>, GraphEntry> graphs;
  long graph_replays = 0, graph_captures_failed = 0;
  int graph_count = 0;          // instantiated graphs alive (capped at 32 shapes)
  hipStream_t cap_stream = nullptr;   // private stream for captures (the caller's may be the legacy default stream)
  DevBuf lens;          // 4 * maxB ints: len0, len1, len2, enc_len
  DevBuf rsbuf, op_rs;  // per-row 2^-e of the LayerNorm-produced GEMM operand currently in y / yr; gam_op_gemm's
  int* range_flag = nullptr;   // device int: set when an unscaled sp32 tensor left fp16's range (gam_range_flag)

  // profiler
  int prof_on = 0;   // 0 off, 1 every launch, 2 GEMM family only
  std::vector<ProfEvent> prof_events;
  size_t prof_used = 0;
  double prof_work[GAM_PF_NCLASS] = {0};
  double prof_bytes[GAM_PF_NCLASS] = {0};   // algorithmic operand + result bytes (GEMM classes)
  int64_t prof_launches[GAM_PF_NCLASS] = {0};
};

namespace {

int fail(gam_handle* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h) h->err = buf;
  return code;
}

#define HIPCHK(h, expr)                                                                        \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return fail(h, -2, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// Every weight and table of gam_finalize reaches the device here: `alloc_bytes` >= `bytes` of memory that h->owned holds BEFORE anything
// is copied into it (a failed copy leaks nothing), then `bytes` from `src` (NULL: no copy).  NULL: the allocation or the copy failed.
void* dev_upload(gam_handle* h, const void* src, size_t bytes, size_t alloc_bytes) {
  h->owned.emplace_back();
  DevBuf& b = h->owned.back();
  if (b.alloc((alloc_bytes + 3) / 4) != hipSuccess) return nullptr;
  if (src && bytes && hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  return b.p;
}

float* upload(gam_handle* h, const std::vector<float>& v) {
  return (float*)dev_upload(h, v.data(), v.size() * sizeof(float), std::max<size_t>(v.size(), 4) * sizeof(float));
}

// Grow-only: a buffer that already holds `floats` is left alone.  A workspace buffer that moves invalidates the captured graphs, which
// hold its old pointer (ws_generation); the tables a kernel receives as launch arguments of a decode call do not (ensure_table).
int ensure_table(gam_handle* h, DevBuf& b, size_t floats) {
  if (floats <= b.cap) return 0;
  HIPCHK(h, b.alloc(floats));
  return 0;
}

int ensure(gam_handle* h, DevBuf& b, size_t floats) {
  if (floats <= b.cap) return 0;
  if (int r = ensure_table(h, b, floats)) return r;
  ++h->ws_generation;
  return 0;
}

uint16_t float_to_half_bits(float f) {   // round to nearest even, subnormals kept
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x >= 0x7f800000u) return (uint16_t)(sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u));
  if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // rounds to >= 65520 -> inf
  if (x < 0x38800000u) {                                      // below 2^-14: subnormal half
    if (x < 0x33000000u) return (uint16_t)sign;               // < 2^-25 -> 0
    const int e = (int)(x >> 23);
    uint32_t m = (x & 0x7fffffu) | 0x800000u;
    const int shift = 126 - e;                                // 14..24
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    m >>= shift;
    if (rem > half || (rem == half && (m & 1u))) ++m;
    return (uint16_t)(sign | m);
  }
  const uint32_t e = (x >> 23) - 112u;
  uint32_t m = x & 0x7fffffu;
  uint32_t h = (e << 10) | (m >> 13);
  const uint32_t rem = m & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;
  return (uint16_t)(sign | h);
}

float half_to_float(uint16_t x) {
  const uint32_t sign = (x >> 15) & 1, exp = (x >> 10) & 0x1f, man = x & 0x3ff;
  uint32_t f;
  if (exp == 0) {
    if (man == 0) f = sign << 31;
    else {
      int e = -1; uint32_t m = man;
      do { ++e; m <<= 1; } while (!(m & 0x400));
      f = (sign << 31) | ((uint32_t)(127 - 15 - e) << 23) | ((m & 0x3ff) << 13);
    }
  } else if (exp == 31) f = (sign << 31) | 0x7f800000u | (man << 13);
  else f = (sign << 31) | ((exp + 127 - 15) << 23) | (man << 13);
  float r; memcpy(&r, &f, 4); return r;
}

// W * 2^shift = hi + lo with hi, lo in fp16; the power-of-two scale puts max|W| near 2^8 so
// that lo (~2^-11 |W|) stays in the normal fp16 range for all but negligible entries.  K = the reduction length (row
// pitch of W): the sp32 copy exists when K % 32 == 0.
// conv_taps > 0 (K = conv_taps * C, k = tap * C + c): the sp32 copy orders its k-tiles (32-channel block, tap) -- taps
// innermost, the order gam_gemm_sp_kernel walks an implicit-GEMM A operand in; the h16 plane does the same with 64-channel blocks.
int make_split(gam_handle* h, const std::vector<float>& w, W16& out, int K = 0, int conv_taps = 0) {
  float mx = 0.f;
  for (float v : w) mx = std::max(mx, fabsf(v));
  int shift = 0;
  if (mx > 0.f && std::isfinite(mx)) shift = (int)floorf(log2f(256.0f / mx));
  shift = std::max(-24, std::min(24, shift));
  const float sc = ldexpf(1.0f, shift);
  std::vector<uint16_t> hi(w.size()), lo(w.size());
  for (size_t i = 0; i < w.size(); ++i) {
    const float v = w[i] * sc;
    const uint16_t hb = float_to_half_bits(v);
    hi[i] = hb;
    lo[i] = float_to_half_bits(v - half_to_float(hb));
  }
  out.inv = ldexpf(1.0f, -shift);
  std::vector<uint16_t> hp(hi);
  if (conv_taps > 0 && K > 0 && (K / conv_taps) % 64 == 0 && w.size() % (size_t)K == 0) {
    // one-term kernel, implicit-GEMM A operand: k-tile = 64 channels of one tap, taps innermost within a 64-channel block
    const size_t C = (size_t)K / conv_taps, cb64 = C / 64;
    for (size_t n = 0; n < w.size() / K; ++n)
      for (size_t cb = 0; cb < cb64; ++cb)
        for (size_t t = 0; t < (size_t)conv_taps; ++t)
          for (size_t j = 0; j < 64; ++j)
            hp[n * K + (cb * conv_taps + t) * 64 + j] = hi[n * K + t * C + cb * 64 + j];
  }
  out.h16 = (_Float16*)dev_upload(h, hp.data(), w.size() * 2, std::max<size_t>(w.size(), 8) * 2 + 64);
  if (!out.h16) return -2;
  if (K > 0 && K % 32 == 0 && w.size() % (size_t)K == 0) {
    // the same planes in the sp32 layout: row n, k-block kb -> [hi x32 | lo x32] (gam_gemm_sp.h)
    std::vector<uint16_t> sp(w.size() * 2);
    for (size_t i = 0; i < w.size(); ++i) {
      const size_t n = i / K, k = i % K;
      size_t kb = k / 32;
      if (conv_taps > 0) {
        const size_t cblocks = (size_t)K / conv_taps / 32, t = kb / cblocks, cb = kb % cblocks;
        kb = cb * conv_taps + t;
      }
      const size_t o = n * 2 * (size_t)K + kb * 64 + (k % 32);
      sp[o] = hi[i];
      sp[o + 32] = lo[i];
    }
    out.sp = (_Float16*)dev_upload(h, sp.data(), sp.size() * 2, sp.size() * 2 + 64);
    if (!out.sp) return -2;
  }
  return 0;
}

const HostTensor* find(gam_handle* h, const std::string& key) {
  auto it = h->staged.find(key);
  return it == h->staged.end() ? nullptr : &it->second;
}

// ---- profiler: one event pair per launch, on the launch stream ----
struct ProfScope {
  gam_handle* h;
  hipStream_t s;
  ProfEvent* ev = nullptr;
  ProfScope(gam_handle* h_, hipStream_t s_, int cls, double work) : h(h_), s(s_) {
    if (!h->prof_on || (h->prof_on == 2 && cls != GAM_PF_GEMM && cls != GAM_PF_CONV2)) return;
    if (h->prof_used == h->prof_events.size()) {
      ProfEvent e;
      if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
      h->prof_events.push_back(e);
    }
    ev = &h->prof_events[h->prof_used++];
    ev->cls = cls;
    h->prof_work[cls] += work;
    h->prof_launches[cls] += 1;
    hipEventRecord(ev->a, s);
  }
  ~ProfScope() {
    if (ev) hipEventRecord(ev->b, s);
  }
};

// A split-K reduce left to the consumer: the LayerNorm that follows a residual GEMM sums the slices itself (gam_norm.h).
// The record carries everything the stand-alone reduce pass would need (`full` + `act`), so a consumer that does not match
// what was deferred -- another x, another shape, a GEMM launched in between -- gets the reduce kernel instead of stale sums.
struct PendingReduce {
  const float* part = nullptr;
  int nsplit = 0;
  const float* bias = nullptr;
  const float* resid = nullptr;
  float alpha = 1.0f;
  GamGemmArgs full;     // the GEMM as launched without split-K: C / M / N / ldc identify the consumer that may fuse
  int act = 0;
  void clear() { part = nullptr; nsplit = 0; }
};

// run the deferred reduce as its own pass (the fall-back of every path that cannot fuse it)
int flush_pending(gam_handle* h, hipStream_t s, PendingReduce* p) {
  if (p == nullptr || p->part == nullptr) return 0;
  const hipError_t e = gam_launch_splitk_reduce(p->full, p->act, p->nsplit, s);
  const int M = p->full.M, N = p->full.N;
  p->clear();
  if (e != hipSuccess) return fail(h, -2, "split-K reduce launch (M=%d N=%d): %s", M, N, hipGetErrorString(e));
  return 0;
}

// the split-fp16 arithmetic family: GAM_GEMM_F16X3 (three terms, fp32-equivalent, the default) and GAM_GEMM_F16 (one term, opt-in)
static inline bool split_mode(const gam_handle* h) { return h->gemm_mode != GAM_GEMM_F32; }

int gemm(gam_handle* h, hipStream_t s, const GamGemmArgs& a_in, int act, int cls = GAM_PF_GEMM, const W16* w16 = nullptr,
         PendingReduce* defer = nullptr) {
  GamGemmArgs a = a_in;
  if (int r = flush_pending(h, s, defer)) return r;   // (an unconsumed deferral must not be overwritten: its C would stay unreduced)
  a.range_flag = h->use_range ? h->range_flag : nullptr;
  if (!split_mode(h)) a.c_guard = 0;   // fp32 consumers have no range limit
  ProfScope ps(h, s, cls, 2.0 * (double)a.M * (double)a.N * (double)a.K);
  if (ps.ev) {   // unique bytes: A (overlapping rows counted once), W, C (+ residual)
    const double abytes = a.a_mode == 0 ? ((double)(a.M - 1) * (double)std::min<long>(a.lda, a.K) + a.K) * 4.0
                                        : (double)a.M / a.conv_f2 * 2.0 * a.conv_fp * a.conv_c * 4.0;
    h->prof_bytes[cls] += abytes * (a.n_switch > 0 ? 2.0 : 1.0) + 4.0 * a.N * a.K + 4.0 * a.M * a.N * (a.R ? 2.0 : 1.0);   // (n_switch: two A operands)
  }
  hipError_t e;
  if (a.Asp != nullptr) {   // split-fp16 operands: gam_gemm_sp_kernel
    if (!split_mode(h)) return fail(h, -2, "sp32 A operand outside the split-fp16 GEMM mode");
    if (w16 == nullptr || w16->sp == nullptr) return fail(h, -2, "sp32 A without sp32 W planes");
    a.wscale_inv = w16->inv;
    a.Wsp = w16->sp;
    a.h16 = 0;
    if (a.a_fmt == 2) {
      // one fp16 MFMA per product: plain-fp16 operands (the producers wrote format 2), and the kernel is told HALF the
      // reduction length -- 64 fp16 values fill the 128-byte line that holds 32 (hi, lo) pairs in the three-term layout
      if (a.K % 64 != 0 || (a.a_mode == 0 ? a.lda % 64 != 0 : a.conv_c % 64 != 0) || w16->h16 == nullptr)
        return fail(h, -2, "GAM_GEMM_F16: K / row pitch of a GEMM operand is not a multiple of 64 (M=%d N=%d K=%d)", a.M, a.N, a.K);
      a.h16 = 1; a.K /= 2; a.lda /= 2; a.conv_c /= 2;
      a.Wsp = w16->h16;
    }
    GamSpPlan plan = gam_gemm_sp_plan(a.M, a.N, a.K, a.a_mode, h->ncu);
    if (!h->use_splitk) plan.s = 1;   // GAM_SPLITK=0: the A/B switch covers this path too (tile shape as planned)
    a.sp_mt = plan.mt; a.sp_nw = plan.nw; a.sp_ns = plan.ns;
    GamGemmArgs full = a;
    if (plan.s > 1) {   // small grid: S slices of K leave partial sums, the reduce pass applies the epilogue
      if (int r = ensure(h, h->splitk_ws, (size_t)plan.s * a.M * a.N + 64)) return r;
      a.splitk = plan.s; a.partial = h->splitk_ws.p;
    }
    e = gam_launch_gemm_sp(a, act, s);
    if (e != hipSuccess) return fail(h, -2, "sp gemm launch (M=%d N=%d K=%d): %s", a.M, a.N, a.K, hipGetErrorString(e));
    if (plan.s > 1 && defer != nullptr && h->fuse_reduce && act == GAM_ACT_NONE && !a.c_split && !a.c_guard && a.lens == nullptr &&
        !a.remap && a.ldc == a.N && a.bias != nullptr && a.R != nullptr && a.ldr == a.N) {   // (the fused row builder takes both as given)
      defer->part = a.partial; defer->nsplit = plan.s; defer->bias = a.bias; defer->resid = a.R; defer->alpha = a.alpha;
      defer->full = full; defer->full.partial = a.partial; defer->act = act;
    } else if (plan.s > 1) {
      full.partial = a.partial;
      e = gam_launch_splitk_reduce(full, act, plan.s, s);
      if (e != hipSuccess) return fail(h, -2, "split-K reduce launch (M=%d N=%d): %s", a.M, a.N, hipGetErrorString(e));
    }
    return 0;
  }
  // Everything else runs on the exact-fp32 kernel: the exact mode, the decode heads, and the split modes' GEMMs without sp32
  // operands (shapes the LDS-DMA kernel cannot take).  Its A is never row-scaled and its C is fp32.
  if (a.a_rs != nullptr || a.c_split) return fail(h, -2, "row-scaled A or split C without sp32 operands (M=%d N=%d K=%d)", a.M, a.N, a.K);
  // Split-K for grids that would leave most CUs idle (single clips, short batches: 126 tokens x 768
  // columns = 6 tiles): S slices of K write partial sums, a second pass sums them in a fixed order
  // (bit-reproducible) and applies the epilogue.
  int S = 1;
  if (h->use_splitk && a.a_mode == 0 && a.K % 32 == 0) {
    const int tiles = gam_cdiv(a.M, 128) * gam_cdiv(a.N, 128), nk = a.K / 32, ncu = 256;
    if (tiles * 2 <= ncu && nk >= 4) {
      S = std::min(16, std::min(ncu / tiles, nk / 2));
      while (S > 1 && nk % S != 0) --S;
    }
  }
  GamGemmArgs full = a;
  if (S > 1) {
    DevBuf& ws = cls == GAM_PF_DECODE ? h->dec_splitk_ws : h->splitk_ws;
    if (int r = ensure(h, ws, (size_t)S * a.M * a.N + 64)) return r;
    a.splitk = S; a.ldw = a.K; a.K = a.K / S; a.partial = ws.p;
  }
  e = gam_launch_gemm(a, act, s);
  if (e != hipSuccess) return fail(h, -2, "gemm launch (M=%d N=%d K=%d): %s", a.M, a.N, a.K, hipGetErrorString(e));
  if (S > 1) {
    full.partial = a.partial;
    e = gam_launch_splitk_reduce(full, act, S, s);
    if (e != hipSuccess) return fail(h, -2, "split-K reduce launch (M=%d N=%d): %s", a.M, a.N, hipGetErrorString(e));
  }
  return 0;
}

GamGemmArgs gemm_args(const float* A, long lda, const float* W, const float* bias, float* C, long ldc, int M, int N, int K) {
  GamGemmArgs g;
  memset(&g, 0, sizeof g);
  g.A = A; g.W = W; g.bias = bias; g.C = C; g.R = nullptr;
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldc = ldc; g.ldr = ldc; g.alpha = 1.0f;
  g.rpb = 1; g.fdiv = 1;
  return g;
}

int layernorm(gam_handle* h, hipStream_t s, GamLnArgs a, int mode, PendingReduce* pend = nullptr) {
  if (pend != nullptr && pend->part != nullptr) {
    // fuse only what was deferred for THIS consumer: the LayerNorm's input is the GEMM's C, same rows x columns, dense
    const GamGemmArgs& g = pend->full;
    if (a.x == g.C && a.rows == g.M && a.d == g.N && g.ldc == g.N) {
      a.part = pend->part; a.nsplit = pend->nsplit; a.pbias = pend->bias; a.presid = pend->resid; a.palpha = pend->alpha;
      a.xstore = const_cast<float*>(a.x);
      pend->clear();     // consumed: nothing may fuse (or flush) these slices again
    } else if (int r = flush_pending(h, s, pend)) {
      return r;
    }
  }
  const double bytes = (double)a.rows * a.d * 4.0 * (mode == 0 ? 2.0 : 3.0);
  ProfScope ps(h, s, GAM_PF_NORM, bytes);
  hipError_t e = gam_launch_layernorm(a, mode, s);
  if (e != hipSuccess) return fail(h, -2, "layernorm launch: %s", hipGetErrorString(e));
  return 0;
}

int64_t half_up(int64_t l) { return l <= 0 ? 0 : (l + 1) / 2; }

// Orders a decode-class call behind the previous decode-class call of the handle when the two run on different streams, and records its
// own completion for the next one (see gam_handle::dec_evt).  Same stream: no wait is enqueued, stream order does it.
struct DecodeScope {
  gam_handle* h;
  hipStream_t s;
  DecodeScope(gam_handle* h_, hipStream_t s_) : h(h_), s(s_) {
    if (h->dec_evt == nullptr && hipEventCreateWithFlags(&h->dec_evt, hipEventDisableTiming) != hipSuccess) { h->dec_evt = nullptr; (void)hipGetLastError(); }
    if (h->dec_evt != nullptr && h->dec_evt_set && h->dec_stream != s) (void)hipStreamWaitEvent(s, h->dec_evt, 0);
  }
  ~DecodeScope() {
    if (h->dec_evt != nullptr && hipEventRecord(h->dec_evt, s) == hipSuccess) { h->dec_stream = s; h->dec_evt_set = true; }
  }
};

// The preamble of a decode-class entry point: the stream `s`, the null-handle check, the handle's device made current (before the scope:
// its event belongs to that device) and the DecodeScope.  Checks an entry point makes BEFORE the scope stand in front of it.
#define GAM_DECODE_ENTRY(h, stream)      \
  hipStream_t s = (hipStream_t)(stream); \
  if (!(h)) return -1;                   \
  HIPCHK(h, hipSetDevice((h)->device));  \
  DecodeScope ds(h, s)

// The head precondition of an entry point, made BEFORE GAM_DECODE_ENTRY (a refused call opens no DecodeScope): the handle is finalized
// (`who` opens that message; NULL: the entry point does not ask) and carries the head `want` (GAM_HEAD_CTC / _RNNT / _EMO).
int head_check(gam_handle* h, int want, const char* who) {
  if (!h) return -1;
  if (who && !h->finalized) return fail(h, -1, "%s before gam_finalize", who);
  if (h->cfg.head_type != want || !h->has_head)
    return fail(h, -1, "model has no %s head", want == GAM_HEAD_CTC ? "CTC" : want == GAM_HEAD_RNNT ? "RNN-T" : "emotion");
  return 0;
}

// The RNN-T head's weights as kernel arguments: the predictor's, the joint's.  For every argument struct that names these fields (the
// structs' layouts are their kernels' own).
template <class Args> void rnnt_pred_weights(const gam_handle* h, Args& a) {
  a.gate_tab = h->lstm_tab; a.whh_t = h->lstm_whh_t; a.wih_x = h->lstm_wih_x; a.whh_x = h->lstm_whh_x; a.bias_x = h->lstm_bias_x;
}
template <class Args> void rnnt_joint_weights(const gam_handle* h, Args& a) {
  a.wpred_t = h->jn_pred_t; a.bpred = h->jn_pred_b; a.wout = h->jn_out_w; a.bout = h->jn_out_b;
}

}  // namespace

// ===================================================================================
extern "C" {

int gam_abi_version(void) { return GAM_ABI_VERSION; }

const char* gam_last_error(const gam_handle* h) { return h ? h->err.c_str() : "null handle"; }

int gam_create(const gam_config* cfg, int device_id, gam_handle** out) {
  if (!cfg || !out) return -1;
  gam_handle* h = new gam_handle();
  h->cfg = *cfg;
  h->device = device_id;
  *out = h;
  if (const char* e = getenv("GAM_SPLITK")) h->use_splitk = atoi(e);
  if (const char* e = getenv("GAM_PACK")) h->use_pack = atoi(e);
  if (const char* e = getenv("GAM_FUSE_REDUCE")) h->fuse_reduce = atoi(e);
  if (const char* e = getenv("GAM_GRAPH")) h->use_graph = atoi(e);
  if (const char* e = getenv("GAM_GRAPH_MAX_ROWS")) h->graph_max_rows = atoi(e);
  if (const char* e = getenv("GAM_RNNT_CLUSTER")) h->rnnt_cluster = std::max(-1, std::min(8, atoi(e)));   // (the range gam_set_rnnt_cluster accepts)
  if (const char* e = getenv("GAM_RNNT_ALIGN_WS")) h->ra_ws_limit = (size_t)std::max(1ll, atoll(e));
  if (const char* e = getenv("GAM_CTC_ALIGN_WS")) h->al_ws_limit = (size_t)std::max(1ll, atoll(e));
  if (const char* e = getenv("GAM_RNNT_EXCLUSIVE")) h->rnnt_exclusive = atoi(e);
  if (const char* e = getenv("GAM_RNNT_COOP")) h->rnnt_coop = atoi(e);
  if (const char* e = getenv("GAM_RNNT_FORCE_TIMEOUT")) h->rnnt_force_timeout = atoi(e);
  if (const char* e = getenv("GAM_RNNT_NO_REPAIR")) h->rnnt_no_repair = atoi(e);
  {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && n > 0) h->ncu = n;
    int co = 0;
    if (hipDeviceGetAttribute(&co, hipDeviceAttributeCooperativeLaunch, device_id) != hipSuccess || co == 0) h->rnnt_coop = 0;
  }
  if (const char* e = getenv("GAM_ROWSCALE")) h->use_rowscale = atoi(e);
  if (const char* e = getenv("GAM_RANGE")) h->use_range = atoi(e);
  if (const char* e = getenv("GAM_GEMM_MODE"))
    h->gemm_mode = strcmp(e, "f32") == 0 ? GAM_GEMM_F32 : (strcmp(e, "f16") == 0 ? GAM_GEMM_F16 : GAM_GEMM_F16X3);
  const gam_config& c = h->cfg;
  if (c.d_model <= 0 || c.n_heads <= 0 || c.d_model % c.n_heads != 0)
    return fail(h, -1, "bad d_model/n_heads %d/%d", c.d_model, c.n_heads);
  if (c.d_model / c.n_heads != GAM_ATT_DK) return fail(h, -1, "head dim %d unsupported (kernels are built for %d)", c.d_model / c.n_heads, GAM_ATT_DK);
  if (c.d_model % 64 != 0 || c.d_model > 1024) return fail(h, -1, "d_model %d unsupported", c.d_model);
  if (c.subsampling_factor != 4) return fail(h, -1, "subsampling_factor %d unsupported", c.subsampling_factor);
  if (c.subsampling == GAM_SUBS_CONV2D && c.subs_kernel_size != 3) return fail(h, -1, "conv2d stem needs kernel 3");
  if (c.subsampling == GAM_SUBS_CONV1D && c.subs_kernel_size != 5) return fail(h, -1, "conv1d stem needs kernel 5");
  if (c.win_length != c.n_fft) return fail(h, -1, "win_length != n_fft unsupported");
  if (c.n_mels > 64 || c.n_mels != c.feat_in) return fail(h, -1, "n_mels %d / feat_in %d unsupported", c.n_mels, c.feat_in);
  if (c.head_type == GAM_HEAD_RNNT && (c.pred_rnn_layers < 1 || c.pred_rnn_layers > 4 || c.pred_hidden > GAM_RNNT_MAXH || c.joint_hidden > GAM_RNNT_MAXH || c.num_classes > GAM_RNNT_MAXV || c.joint_hidden % 16 != 0 || c.pred_hidden % 16 != 0))
    return fail(h, -1, "RNN-T head shape unsupported");
  if (hipSetDevice(device_id) != hipSuccess) return fail(h, -2, "hipSetDevice(%d) failed", device_id);
  return 0;
}

void gam_destroy(gam_handle* h) {
  if (!h) return;
  hipSetDevice(h->device);
  for (auto& e : h->prof_events) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
  for (auto& g : h->graphs)
    if (g.second.exec) hipGraphExecDestroy(g.second.exec);
  if (h->cap_stream) hipStreamDestroy(h->cap_stream);
  if (h->dec_evt) hipEventDestroy(h->dec_evt);
  if (getenv("GAM_GRAPH_DEBUG")) fprintf(stderr, "[gam] graph replays %ld, failed captures %ld\n", h->graph_replays, h->graph_captures_failed);
  delete h;   // every device buffer is a DevBuf member or sits in `owned`: they free themselves
}

int gam_set_weight(gam_handle* h, const char* key, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
  if (!h || !key || !host_ptr) return -1;
  if (h->finalized) return fail(h, -1, "gam_set_weight after gam_finalize");
  HostTensor t;
  for (int i = 0; i < ndim; ++i) t.shape.push_back(shape[i]);
  const int64_t n = t.numel();
  t.data.resize((size_t)n);
  switch (dtype) {
    case GAM_DTYPE_F32: memcpy(t.data.data(), host_ptr, (size_t)n * 4); break;
    case GAM_DTYPE_F16: for (int64_t i = 0; i < n; ++i) t.data[i] = half_to_float(((const uint16_t*)host_ptr)[i]); break;
    case GAM_DTYPE_BF16: for (int64_t i = 0; i < n; ++i) { uint32_t u = (uint32_t)((const uint16_t*)host_ptr)[i] << 16; memcpy(&t.data[i], &u, 4); } break;
    case GAM_DTYPE_F64: for (int64_t i = 0; i < n; ++i) t.data[i] = (float)((const double*)host_ptr)[i]; break;
    case GAM_DTYPE_I64: for (int64_t i = 0; i < n; ++i) t.data[i] = (float)((const int64_t*)host_ptr)[i]; break;
    default: return fail(h, -1, "unknown dtype %d for %s", dtype, key);
  }
  h->staged[key] = std::move(t);
  return 0;
}

// -----------------------------------------------------------------------------------
// gam_finalize (DESIGN.md "Finalize pieces"): the staged host tensors become device weights.  A sequence of named pieces with explicit
// inputs; each returns 0 or the code of its fail().
//   fin_frontend                        DFT basis, mel filterbank (given, or mel_fallback), band table
//   fin_stem_conv2d | fin_stem_conv1d   the subsampling stem's operands
//   fin_layer                           one Conformer layer, (h, index) -> LayerW; fin_qkv and fin_conv_norm are its two non-trivial members
//   fin_rotary | fin_rel_pos            the position table of the attention variant
//   fin_head                            CTC / emotion: one upload_linear; RNN-T: fin_rnnt_head (lstm_input_table, fin_rnnt_upper)
struct Dst {   // where the device pointer of an upload goes, and the name its failure message carries
  float** p;
  const char* name;
};
#define DST(member) Dst{&(member), #member}

static int need(gam_handle* h, const std::string& key, int64_t n, const HostTensor** t) {
  *t = find(h, key);
  if (!*t) return fail(h, -3, "missing weight %s", key.c_str());
  if ((*t)->numel() != n) return fail(h, -3, "weight %s has %lld elements, expected %lld", key.c_str(), (long long)(*t)->numel(), (long long)n);
  return 0;
}

static int upload_to(gam_handle* h, Dst dst, const std::vector<float>& v) {
  *dst.p = upload(h, v);
  return *dst.p ? 0 : fail(h, -2, "device upload failed (%s)", dst.name);
}

static int up_split(gam_handle* h, const std::vector<float>& w, W16* out, int K, int conv_taps = 0) {
  return make_split(h, w, *out, K, conv_taps) ? fail(h, -2, "split upload failed") : 0;
}

// <prefix>.weight [nout, nin] and <prefix>.bias [nout] as they are; split != NULL: the weight's split-fp16 operand too (reduction length nin)
static int upload_linear(gam_handle* h, const std::string& prefix, int64_t nout, int64_t nin, Dst w, Dst b, W16* split) {
  const HostTensor *wt, *bt;
  if (int r = need(h, prefix + ".weight", nout * nin, &wt)) return r;
  if (int r = need(h, prefix + ".bias", nout, &bt)) return r;
  if (int r = upload_to(h, w, wt->data)) return r;
  if (int r = upload_to(h, b, bt->data)) return r;
  return split ? up_split(h, wt->data, split, (int)nin) : 0;
}

static int upload_ln(gam_handle* h, const std::string& prefix, int D, Dst w, Dst b) { return upload_linear(h, prefix, D, 1, w, b, nullptr); }

// [r][k] -> [k][r]
static void transpose_rk(const float* in, size_t R, size_t K, float* out) {
  for (size_t r = 0; r < R; ++r)
    for (size_t k = 0; k < K; ++k) out[k * R + r] = in[r * K + k];
}

// [n][a][b] -> [n][b][a]: the two inner axes swapped
static std::vector<float> swap_inner(const std::vector<float>& in, size_t N, size_t A, size_t B) {
  std::vector<float> out(in.size());
  for (size_t n = 0; n < N; ++n) transpose_rk(&in[n * A * B], A, B, &out[n * A * B]);
  return out;
}

// [r][k] -> [k/4][r][4]: four consecutive k of a row side by side, the float4 the cluster decode kernel reads
static std::vector<float> quad_rk(const std::vector<float>& in, size_t R, size_t K) {
  std::vector<float> out(in.size());
  for (size_t r = 0; r < R; ++r)
    for (size_t k = 0; k < K; ++k) out[((k / 4) * R + r) * 4 + (k & 3)] = in[r * K + k];
  return out;
}

// torchaudio melscale_fbanks(htk, norm=None, f_min 0, f_max sr/2) as [nf][n_mels]
static std::vector<float> mel_fallback(const gam_config& c, int nf) {
  std::vector<float> fb((size_t)nf * c.n_mels, 0.f);
  const double fmax = c.sample_rate / 2.0, mmax = 2595.0 * log10(1.0 + fmax / 700.0);
  std::vector<double> fpts(c.n_mels + 2);
  for (int i = 0; i < c.n_mels + 2; ++i) fpts[i] = 700.0 * (pow(10.0, (mmax * i / (c.n_mels + 1)) / 2595.0) - 1.0);
  for (int f = 0; f < nf; ++f) {
    const double fr = (double)(c.sample_rate / 2) * f / (nf - 1);
    for (int m = 0; m < c.n_mels; ++m) {
      const double down = (fr - fpts[m]) / (fpts[m + 1] - fpts[m]), up = (fpts[m + 2] - fr) / (fpts[m + 2] - fpts[m + 1]);
      fb[(size_t)f * c.n_mels + m] = (float)std::max(0.0, std::min(down, up));
    }
  }
  return fb;
}

// window-folded DFT basis + mel filterbank
static int fin_frontend(gam_handle* h) {
  const gam_config& c = h->cfg;
  const int n = c.n_fft, nf = n / 2 + 1;
  h->nf = nf;
  h->kpad = (n + 31) / 32 * 32;
  std::vector<double> win(n);
  if (const HostTensor* w = find(h, "preprocessor.featurizer.0.spectrogram.window")) {
    if (w->numel() != n) return fail(h, -3, "window has %lld taps, expected %d", (long long)w->numel(), n);
    for (int i = 0; i < n; ++i) win[i] = w->data[i];
  } else {
    for (int i = 0; i < n; ++i) win[i] = (double)(float)(0.5 - 0.5 * cos(2.0 * M_PI * i / n));  // periodic hann
  }
  std::vector<float> basis((size_t)2 * nf * h->kpad, 0.f);
  for (int k = 0; k < nf; ++k)
    for (int i = 0; i < n; ++i) {
      const long ki = ((long)k * i) % n;  // exact angle reduction
      const double ang = 2.0 * M_PI * (double)ki / n;
      basis[(size_t)k * h->kpad + i] = (float)(win[i] * cos(ang));
      basis[(size_t)(nf + k) * h->kpad + i] = (float)(-win[i] * sin(ang));
    }
  if (int r = upload_to(h, DST(h->dft_basis), basis)) return r;
  const HostTensor* given = find(h, "preprocessor.featurizer.0.mel_scale.fb");
  if (given && given->numel() != (int64_t)nf * c.n_mels) return fail(h, -3, "mel fb has %lld elements, expected %d", (long long)given->numel(), nf * c.n_mels);
  const std::vector<float> fb = given ? given->data : mel_fallback(c, nf);
  std::vector<int> band(3 * (size_t)c.n_mels, 0);
  std::vector<float> wts;
  for (int m = 0; m < c.n_mels; ++m) {
    int lo = nf, hi = 0;
    for (int f = 0; f < nf; ++f)
      if (fb[(size_t)f * c.n_mels + m] != 0.f) { lo = std::min(lo, f); hi = std::max(hi, f + 1); }
    if (hi <= lo) lo = hi = 0;
    band[3 * m] = lo; band[3 * m + 1] = hi; band[3 * m + 2] = (int)wts.size();
    for (int f = lo; f < hi; ++f) wts.push_back(fb[(size_t)f * c.n_mels + m]);
  }
  h->mel_nw = (int)wts.size();
  if (int r = upload_to(h, DST(h->mel_wts), wts)) return r;
  h->mel_band = (int*)dev_upload(h, band.data(), band.size() * sizeof(int), band.size() * sizeof(int));
  return h->mel_band ? 0 : fail(h, -2, "mel band upload failed");
}

static int fin_stem_conv2d(gam_handle* h) {
  const int C = h->cfg.d_model, D = h->cfg.d_model, F = h->cfg.feat_in;
  const std::string pe = "encoder.pre_encode.";
  h->f1 = (F + 1) / 2;
  h->f2 = (h->f1 + 1) / 2;
  const HostTensor *w0, *b0, *w2, *b2, *wl, *bl;
  if (int r = need(h, pe + "conv.0.weight", (int64_t)C * 9, &w0)) return r;
  if (int r = need(h, pe + "conv.0.bias", C, &b0)) return r;
  if (int r = need(h, pe + "conv.2.weight", (int64_t)C * C * 9, &w2)) return r;
  if (int r = need(h, pe + "conv.2.bias", C, &b2)) return r;
  if (int r = need(h, pe + "out.weight", (int64_t)D * C * h->f2, &wl)) return r;
  if (int r = need(h, pe + "out.bias", D, &bl)) return r;
  if (int r = upload_to(h, DST(h->c1_w), w0->data)) return r;
  if (int r = upload_to(h, DST(h->c1_b), b0->data)) return r;
  const std::vector<float> t2 = swap_inner(w2->data, C, C, 9);   // [n][c][kh][kw] -> [n][kh*3+kw][c]
  if (int r = upload_to(h, DST(h->c2_w), t2)) return r;
  if (int r = up_split(h, t2, &h->s_c2, 9 * C, C % 32 == 0 ? 9 : 0)) return r;
  if (int r = upload_to(h, DST(h->c2_b), b2->data)) return r;
  const std::vector<float> l = swap_inner(wl->data, D, C, h->f2);   // [n][c][f] -> [n][f][c]: columns c*f2+f -> f*C+c (encoder.py:126-127 flattens channel-major)
  if (int r = upload_to(h, DST(h->lin_w), l)) return r;
  if (int r = up_split(h, l, &h->s_lin, C * h->f2)) return r;
  return upload_to(h, DST(h->lin_b), bl->data);
}

static int fin_stem_conv1d(gam_handle* h) {
  const int C = h->cfg.d_model, F = h->cfg.feat_in, ks = h->cfg.subs_kernel_size;
  const std::string pe = "encoder.pre_encode.";
  const HostTensor *w0, *b0, *w2, *b2;
  if (int r = need(h, pe + "conv.0.weight", (int64_t)C * F * ks, &w0)) return r;
  if (int r = need(h, pe + "conv.0.bias", C, &b0)) return r;
  if (int r = need(h, pe + "conv.2.weight", (int64_t)C * C * ks, &w2)) return r;
  if (int r = need(h, pe + "conv.2.bias", C, &b2)) return r;
  const std::vector<float> r0 = swap_inner(w0->data, C, F, ks), r2 = swap_inner(w2->data, C, C, ks);   // [n][f][k] -> [n][k][f]
  if (int r = upload_to(h, DST(h->c1_w), r0)) return r;
  if (int r = up_split(h, r0, &h->s_c1, ks * F)) return r;
  if (int r = upload_to(h, DST(h->c1_b), b0->data)) return r;
  if (int r = upload_to(h, DST(h->c2_w), r2)) return r;
  if (int r = up_split(h, r2, &h->s_c2, ks * C)) return r;
  return upload_to(h, DST(h->c2_b), b2->data);
}

// rows [W_q; W_k; W_v] and their biases as one operand
static int fin_qkv(gam_handle* h, const std::string& p, LayerW& L) {
  const int D = h->cfg.d_model;
  const HostTensor *wq, *bq, *wk, *bk, *wv, *bv;
  if (int r = need(h, p + "self_attn.linear_q.weight", (int64_t)D * D, &wq)) return r;
  if (int r = need(h, p + "self_attn.linear_q.bias", D, &bq)) return r;
  if (int r = need(h, p + "self_attn.linear_k.weight", (int64_t)D * D, &wk)) return r;
  if (int r = need(h, p + "self_attn.linear_k.bias", D, &bk)) return r;
  if (int r = need(h, p + "self_attn.linear_v.weight", (int64_t)D * D, &wv)) return r;
  if (int r = need(h, p + "self_attn.linear_v.bias", D, &bv)) return r;
  std::vector<float> w(wq->data), b(bq->data);
  w.insert(w.end(), wk->data.begin(), wk->data.end());
  w.insert(w.end(), wv->data.begin(), wv->data.end());
  b.insert(b.end(), bk->data.begin(), bk->data.end());
  b.insert(b.end(), bv->data.begin(), bv->data.end());
  if (int r = upload_to(h, DST(L.wqkv), w)) return r;
  if (int r = upload_to(h, DST(L.bqkv), b)) return r;
  return up_split(h, w, &L.s_wqkv, D);
}

// the conv module's norm as (scale, shift): BatchNorm folded with its running statistics, LayerNorm's affine pair as it is
static int fin_conv_norm(gam_handle* h, const std::string& p, LayerW& L) {
  const int D = h->cfg.d_model;
  const HostTensor *g, *be;
  if (int r = need(h, p + "conv.batch_norm.weight", D, &g)) return r;
  if (int r = need(h, p + "conv.batch_norm.bias", D, &be)) return r;
  if (h->cfg.conv_norm_type != GAM_NORM_BATCH) {
    if (int r = upload_to(h, DST(L.cn_scale), g->data)) return r;
    return upload_to(h, DST(L.cn_shift), be->data);
  }
  const HostTensor *rm, *rv;
  if (int r = need(h, p + "conv.batch_norm.running_mean", D, &rm)) return r;
  if (int r = need(h, p + "conv.batch_norm.running_var", D, &rv)) return r;
  std::vector<float> sc(D), sh(D);
  for (int i = 0; i < D; ++i) {
    const float inv = 1.0f / sqrtf(rv->data[i] + 1e-5f);
    sc[i] = g->data[i] * inv;
    sh[i] = be->data[i] - rm->data[i] * sc[i];
  }
  if (int r = upload_to(h, DST(L.cn_scale), sc)) return r;
  return upload_to(h, DST(L.cn_shift), sh);
}

static int fin_layer(gam_handle* h, int li, LayerW& L) {
  const gam_config& c = h->cfg;
  const int D = c.d_model, DFF = D * c.ff_expansion_factor;
  const std::string p = "encoder.layers." + std::to_string(li) + ".";
  memset(&L, 0, sizeof L);
  if (int r = upload_ln(h, p + "norm_feed_forward1", D, DST(L.ln_ff1_w), DST(L.ln_ff1_b))) return r;
  if (int r = upload_linear(h, p + "feed_forward1.linear1", DFF, D, DST(L.ff1_w1), DST(L.ff1_b1), &L.s_ff1_w1)) return r;
  if (int r = upload_linear(h, p + "feed_forward1.linear2", D, DFF, DST(L.ff1_w2), DST(L.ff1_b2), &L.s_ff1_w2)) return r;
  if (int r = upload_ln(h, p + "norm_self_att", D, DST(L.ln_att_w), DST(L.ln_att_b))) return r;
  if (int r = fin_qkv(h, p, L)) return r;
  if (int r = upload_linear(h, p + "self_attn.linear_out", D, D, DST(L.wo), DST(L.bo), &L.s_wo)) return r;
  if (c.self_attention_model == GAM_ATT_REL_POS) {
    const HostTensor *wp, *pu, *pv;
    if (int r = need(h, p + "self_attn.linear_pos.weight", (int64_t)D * D, &wp)) return r;
    if (int r = need(h, p + "self_attn.pos_bias_u", D, &pu)) return r;
    if (int r = need(h, p + "self_attn.pos_bias_v", D, &pv)) return r;
    if (int r = upload_to(h, DST(L.wpos), wp->data)) return r;
    if (int r = up_split(h, wp->data, &L.s_wpos, D)) return r;
    if (int r = upload_to(h, DST(L.pos_u), pu->data)) return r;
    if (int r = upload_to(h, DST(L.pos_v), pv->data)) return r;
  }
  if (int r = upload_ln(h, p + "norm_conv", D, DST(L.ln_conv_w), DST(L.ln_conv_b))) return r;
  if (int r = upload_linear(h, p + "conv.pointwise_conv1", 2 * D, D, DST(L.pw1_w), DST(L.pw1_b), &L.s_pw1)) return r;
  if (int r = upload_linear(h, p + "conv.depthwise_conv", D, c.conv_kernel_size, DST(L.dw_w), DST(L.dw_b), nullptr)) return r;
  if (int r = fin_conv_norm(h, p, L)) return r;
  if (int r = upload_linear(h, p + "conv.pointwise_conv2", D, D, DST(L.pw2_w), DST(L.pw2_b), &L.s_pw2)) return r;
  if (int r = upload_ln(h, p + "norm_feed_forward2", D, DST(L.ln_ff2_w), DST(L.ln_ff2_b))) return r;
  if (int r = upload_linear(h, p + "feed_forward2.linear1", DFF, D, DST(L.ff2_w1), DST(L.ff2_b1), &L.s_ff2_w1)) return r;
  if (int r = upload_linear(h, p + "feed_forward2.linear2", D, DFF, DST(L.ff2_w2), DST(L.ff2_b2), &L.s_ff2_w2)) return r;
  return upload_ln(h, p + "norm_out", D, DST(L.ln_out_w), DST(L.ln_out_b));
}

// rotary table (encoder.py:342-355; base = pos_emb_max_len)
static int fin_rotary(gam_handle* h) {
  const int dk = h->cfg.d_model / h->cfg.n_heads, half = dk / 2, n = h->cfg.pos_emb_max_len;
  std::vector<float> cs((size_t)n * half), sn((size_t)n * half);
  for (int i = 0; i < half; ++i) {
    const float inv_freq = 1.0f / powf((float)n, (float)(2 * i) / (float)dk);
    for (int t = 0; t < n; ++t) {
      const float fr = (float)t * inv_freq;
      cs[(size_t)t * half + i] = (float)cos((double)fr);
      sn[(size_t)t * half + i] = (float)sin((double)fr);
    }
  }
  if (int r = upload_to(h, DST(h->rot_cos), cs)) return r;
  return upload_to(h, DST(h->rot_sin), sn);
}

// RelPositionalEmbedding.create_pe (encoder.py:312-327): pe(r)[2i] = sin(r * w_i), pe(r)[2i+1] = cos(r * w_i),
// w_i = exp(2i * -(ln 10000 / D)); rows ascending in r
static int fin_rel_pos(gam_handle* h) {
  const int D = h->cfg.d_model, n = h->cfg.pos_emb_max_len;
  std::vector<float> pe((size_t)(2 * n - 1) * D);
  for (int i = 0; i < D / 2; ++i) {
    const float w = expf((float)(2 * i) * (float)(-(log(10000.0) / D)));
    for (int r = -(n - 1); r <= n - 1; ++r) {
      const float ang = (float)r * w;
      pe[(size_t)(r + n - 1) * D + 2 * i] = (float)sin((double)ang);
      pe[(size_t)(r + n - 1) * D + 2 * i + 1] = (float)cos((double)ang);
    }
  }
  if (int r = upload_to(h, DST(h->rel_pe), pe)) return r;
  // its sp32 copy, split by the kernel that splits every other fp32 operand (D % 32 == 0: a row starts on a 32-element block)
  h->rel_pe_sp = (float*)dev_upload(h, nullptr, 0, pe.size() * sizeof(float));
  if (!h->rel_pe_sp) return fail(h, -2, "device upload failed (h->rel_pe_sp)");
  hipLaunchKernelGGL(gam_to_sp32_kernel, dim3((int)std::min<size_t>((pe.size() / 4 + 255) / 256, 4096)), dim3(256), 0, nullptr, h->rel_pe,
                     reinterpret_cast<_Float16*>(h->rel_pe_sp), pe.size() / 4, (const float*)nullptr, D);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(nullptr));
  return 0;
}

// nn.LSTM layers 1 .. L-1 (decoder.py:78-83): transposed like W_hh, biases summed
static int fin_rnnt_upper(gam_handle* h) {
  const int PH = h->cfg.pred_hidden, LX = h->cfg.pred_rnn_layers - 1;
  const size_t G = (size_t)4 * PH;
  std::vector<float> wih_x(LX * PH * G), whh_x(LX * PH * G), bias_x(LX * G);
  for (int l = 1; l <= LX; ++l) {
    const std::string sfx = "_l" + std::to_string(l);
    const HostTensor *wi, *wh, *bi, *bh;
    if (int r = need(h, "head.decoder.lstm.weight_ih" + sfx, (int64_t)4 * PH * PH, &wi)) return r;
    if (int r = need(h, "head.decoder.lstm.weight_hh" + sfx, (int64_t)4 * PH * PH, &wh)) return r;
    if (int r = need(h, "head.decoder.lstm.bias_ih" + sfx, 4 * PH, &bi)) return r;
    if (int r = need(h, "head.decoder.lstm.bias_hh" + sfx, 4 * PH, &bh)) return r;
    transpose_rk(wi->data.data(), G, PH, &wih_x[(l - 1) * PH * G]);
    transpose_rk(wh->data.data(), G, PH, &whh_x[(l - 1) * PH * G]);
    for (size_t r = 0; r < G; ++r) bias_x[(l - 1) * G + r] = bi->data[r] + bh->data[r];
  }
  if (int r = upload_to(h, DST(h->lstm_wih_x), wih_x)) return r;
  if (int r = upload_to(h, DST(h->lstm_whh_x), whh_x)) return r;
  return upload_to(h, DST(h->lstm_bias_x), bias_x);
}

// The embedding folded into the first LSTM layer's input half: row v = W_ih emb[v] + b_ih + b_hh; row V (no token yet) = the biases
static std::vector<float> lstm_input_table(const HostTensor* emb, const HostTensor* wih, const HostTensor* bih, const HostTensor* bhh, int V, int PH) {
  std::vector<float> tab((size_t)(V + 1) * 4 * PH);
  for (int v = 0; v <= V; ++v)
    for (int r = 0; r < 4 * PH; ++r) {
      float acc = 0.f;
      if (v < V) {
        const float* wr = &wih->data[(size_t)r * PH];
        const float* e = &emb->data[(size_t)v * PH];
        for (int k = 0; k < PH; ++k) acc = fmaf(wr[k], e[k], acc);
      }
      tab[(size_t)v * 4 * PH + r] = (acc + bih->data[r]) + bhh->data[r];
    }
  return tab;
}

static int fin_rnnt_head(gam_handle* h) {
  const gam_config& c = h->cfg;
  const int D = c.d_model, V = c.num_classes, PH = c.pred_hidden, JH = c.joint_hidden;
  const HostTensor *emb, *wih, *whh, *bih, *bhh, *wp, *bp, *we, *bee, *wo, *bo;
  if (int r = need(h, "head.decoder.embed.weight", (int64_t)V * PH, &emb)) return r;
  if (int r = need(h, "head.decoder.lstm.weight_ih_l0", (int64_t)4 * PH * PH, &wih)) return r;
  if (int r = need(h, "head.decoder.lstm.weight_hh_l0", (int64_t)4 * PH * PH, &whh)) return r;
  if (int r = need(h, "head.decoder.lstm.bias_ih_l0", 4 * PH, &bih)) return r;
  if (int r = need(h, "head.decoder.lstm.bias_hh_l0", 4 * PH, &bhh)) return r;
  if (int r = need(h, "head.joint.pred.weight", (int64_t)JH * PH, &wp)) return r;
  if (int r = need(h, "head.joint.pred.bias", JH, &bp)) return r;
  if (int r = need(h, "head.joint.enc.weight", (int64_t)JH * D, &we)) return r;
  if (int r = need(h, "head.joint.enc.bias", JH, &bee)) return r;
  if (int r = need(h, "head.joint.joint_net.1.weight", (int64_t)V * JH, &wo)) return r;
  if (int r = need(h, "head.joint.joint_net.1.bias", V, &bo)) return r;
  if (c.pred_rnn_layers > 1)
    if (int r = fin_rnnt_upper(h)) return r;
  if (int r = upload_to(h, DST(h->lstm_whh_q), quad_rk(whh->data, 4 * PH, PH))) return r;
  if (int r = upload_to(h, DST(h->jn_pred_q), quad_rk(wp->data, JH, PH))) return r;
  if (int r = upload_to(h, DST(h->lstm_tab), lstm_input_table(emb, wih, bih, bhh, V, PH))) return r;
  if (int r = upload_to(h, DST(h->lstm_whh_t), swap_inner(whh->data, 1, 4 * PH, PH))) return r;
  if (int r = upload_to(h, DST(h->jn_pred_t), swap_inner(wp->data, 1, JH, PH))) return r;
  if (int r = upload_to(h, DST(h->jn_pred_b), bp->data)) return r;
  if (int r = upload_to(h, DST(h->jn_pred_w), wp->data)) return r;
  if (int r = upload_to(h, DST(h->jn_enc_w), we->data)) return r;
  if (int r = upload_to(h, DST(h->jn_enc_b), bee->data)) return r;
  if (int r = upload_to(h, DST(h->jn_out_w), wo->data)) return r;
  return upload_to(h, DST(h->jn_out_b), bo->data);
}

static int fin_head(gam_handle* h) {
  const gam_config& c = h->cfg;
  if (c.head_type == GAM_HEAD_CTC) return upload_linear(h, "head.decoder_layers.0", c.num_classes, c.d_model, DST(h->ctc_w), DST(h->ctc_b), nullptr);
  if (c.head_type == GAM_HEAD_EMO) return upload_linear(h, "head", c.num_classes, c.d_model, DST(h->emo_w), DST(h->emo_b), nullptr);
  return c.head_type == GAM_HEAD_RNNT ? fin_rnnt_head(h) : 0;
}

int gam_finalize(gam_handle* h) {
  if (!h) return -1;
  if (h->finalized) return 0;
  HIPCHK(h, hipSetDevice(h->device));
  const gam_config& c = h->cfg;
  if (int r = fin_frontend(h)) return r;
  // A handle may carry only a subset of the operators (e.g. a stand-alone FeatureExtractor or ConformerEncoder module on the Python side).
  const bool build_encoder = find(h, "encoder.pre_encode.conv.0.weight") != nullptr;
  if (build_encoder) {
    if (int r = c.subsampling == GAM_SUBS_CONV2D ? fin_stem_conv2d(h) : fin_stem_conv1d(h)) return r;
    h->layers.resize(c.n_layers);
    for (int li = 0; li < c.n_layers; ++li)
      if (int r = fin_layer(h, li, h->layers[li])) return r;
    if (int r = c.self_attention_model == GAM_ATT_ROTARY ? fin_rotary(h) : fin_rel_pos(h)) return r;
  }
  h->has_encoder = build_encoder;
  h->has_head = find(h, "head.decoder_layers.0.weight") != nullptr || find(h, "head.joint.enc.weight") != nullptr ||
                (c.head_type == GAM_HEAD_EMO && find(h, "head.weight") != nullptr);
  if (h->has_head)
    if (int r = fin_head(h)) return r;
  const std::vector<int> zeros(16, 0);   // the range flag: one int in a 64-byte line of its own
  h->range_flag = (int*)dev_upload(h, zeros.data(), 64, 64);
  if (!h->range_flag) return fail(h, -2, "device upload failed (h->range_flag)");
  h->staged.clear();
  h->finalized = true;
  return 0;
}

int64_t gam_feat_frames(const gam_handle* h, int64_t n) {
  const gam_config& c = h->cfg;
  if (c.center) return n / c.hop_length + 1;
  return n < c.win_length ? 0 : (n - c.win_length) / c.hop_length + 1;
}

int64_t gam_enc_frames(const gam_handle* h, int64_t t) {
  (void)h;
  return half_up(half_up(t));
}

// -----------------------------------------------------------------------------------
int gam_frontend(gam_handle* h, const float* wav, const int64_t* wav_len, int B, int64_t L, float* feat,
                 int64_t* feat_len, void* stream) {
  if (!h || !h->finalized) return fail(h, -1, "gam_frontend before gam_finalize");
  if (B <= 0 || L <= 0) return fail(h, -1, "bad shape B=%d L=%lld", B, (long long)L);
  const gam_config& c = h->cfg;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(h, hipSetDevice(h->device));
  const int hop = c.hop_length, n = c.n_fft, half = n / 2;
  if (c.center && L <= half) return fail(h, -1, "input of %lld samples is too short for reflect padding (%d)", (long long)L, half);
  const int64_t Tf = gam_feat_frames(h, L);
  if (Tf <= 0) return fail(h, -1, "input of %lld samples yields no frames", (long long)L);
  // per-utterance row stride Tfa: row m = b*Tfa + t starts at sample m*hop of the padded buffer
  const int64_t need = (Tf - 1) * hop + h->kpad;
  const int64_t Tfa = (need + hop - 1) / hop;
  const int64_t Lp = Tfa * hop;
  const int lds = (2 * h->nf + 3) / 4 * 4;
  if (int r = ensure(h, h->wavp, (size_t)B * Lp + h->kpad + 64)) return r;
  if (int r = ensure(h, h->spec, (size_t)B * Tfa * lds)) return r;
  {
    ProfScope ps(h, s, GAM_PF_FRONTEND, (double)B * (L + Lp) * 4.0);
    // one extra "utterance row" of zeros is the slack the last rows' K padding reads
    dim3 grid(gam_cdiv(Lp, 256), B);
    hipLaunchKernelGGL(gam_pad_wav_kernel, grid, dim3(256), 0, s, wav, h->wavp.p, B, (long)L, (long)Lp, half, c.center);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemsetAsync(h->wavp.p + (size_t)B * Lp, 0, (h->kpad + 64) * sizeof(float), s));
  }
  GamGemmArgs g = gemm_args(h->wavp.p, hop, h->dft_basis, nullptr, h->spec.p, lds, (int)(B * Tfa), 2 * h->nf, h->kpad);
  // Exact-fp32 MFMA in every mode (like the head GEMMs).  The split-fp16 path assumes O(1) activations: the
  // samples of a quiet frame (|x| ~ 1e-3) leave a_lo in the fp16 subnormal range, the frame's spectrum keeps
  // ~14 bits and its log-mel was off by up to 2e-3 only 50 dB below the frame's own peak (tools/fe_dbg.py;
  // fp32: 1e-4 at 60 dB, the level of an fp32 matmul DFT on the CPU).  21 GFLOP: +70 us per 32 x 20 s batch.
  if (int r = gemm(h, s, g, GAM_ACT_NONE, GAM_PF_FRONTEND, nullptr)) return r;
  {
    GamPowMelArgs a;
    a.spec = h->spec.p; a.wts = h->mel_wts; a.nw = h->mel_nw; a.band = h->mel_band; a.feat = feat; a.wav_len = (const long long*)wav_len; a.feat_len = (long long*)feat_len;
    a.B = B; a.Tfa = (int)Tfa; a.Tf = (int)Tf; a.nf = h->nf; a.n_mels = c.n_mels; a.lds = lds;
    a.hop = hop; a.win = c.win_length; a.center = c.center;
    ProfScope ps(h, s, GAM_PF_FRONTEND, (double)B * Tf * (2.0 * h->nf + c.n_mels) * 4.0);
    dim3 grid(gam_cdiv(Tf, 64), B);
    const size_t pm_lds = (size_t)(64 * (h->nf + 1) + h->mel_nw) * sizeof(float);
    if (pm_lds > 160 * 1024) return fail(h, -1, "n_fft %d: the power / mel kernel's LDS image (%zu bytes) does not fit", c.n_fft, pm_lds);
    if (pm_lds > 64 * 1024) {   // (n_fft > 500; the published frontends need 53 KB)
      static std::atomic<unsigned long long> attr_devs{0};
      HIPCHK(h, gam_set_max_lds(reinterpret_cast<const void*>(gam_powmel_kernel), (int)pm_lds, attr_devs));
    }
    hipLaunchKernelGGL(gam_powmel_kernel, grid, dim3(256), pm_lds, s, a);
    HIPCHK(h, hipGetLastError());
  }
  return 0;
}

// -----------------------------------------------------------------------------------
// The encoder's host path (DESIGN.md "Encoder host path").  encode_impl is a sequence of named pieces with explicit inputs:
//   enc_plan       shape arithmetic and every choice (row layout, operand formats, graph regime); no HIP call
//   enc_workspace  every buffer the call touches, sized from the plan; nothing is allocated behind it
//   enc_lengths -> enc_stem (stem_conv2d | stem_conv1d, + the gather into packed rows)
//   run_layers     ffn_block, attn_block, conv_block, ffn_block, norm_out_block per layer; replay_layers replays it as a hipGraph
//   enc_outputs    channel-first, token-major, lengths
struct EncPlan {
  int B;
  int64_t T;
  int T1, Tv;             // frames after the first / second stride-2 stage
  int Ta, N;              // row stride per utterance of every token-major buffer, N = B * Ta rows in the padded layout
  int NR, Tmax;           // rows the layers run on and rows of the longest utterance: (N, Ta) padded, (valid frames, longest) packed
  int T1a;                // conv1d stem: stage-1 rows per utterance (0 for conv2d)
  int D, DFF, F, H, dk, nl;
  bool conv2d, rel, packed;
  bool sp;                // the encoder GEMMs take sp32 operands (split-fp16 modes, D and DFF multiples of 32)
  int spf;                // operand format the producers write (gam_common.h gam_store4): 0 fp32, 1 (hi, lo) pairs, 2 plain fp16
  bool sp_stem;           // conv1d stem: xin and y1 hold sp32
  bool graph;             // the layer sequence of this shape is captured and replayed (replay_layers)
};

struct EncBufs {          // device pointers into the handle's workspace, valid for this call
  int *len0, *len1, *len2, *elen;   // the lens block
  int *cu, *row_t, *row_src;        // packed rows (gam_pack.h); null in the padded layout
  float* rs;                        // per-row 2^-e of the LayerNorm-produced GEMM operands; null without sp32 operands or GAM_ROWSCALE=0
};

struct EncCtx {           // what a layer block reads; passed by const reference
  EncPlan p;
  EncBufs w;
  GamLnArgs ln;           // the fields every LayerNorm of the layer sequence shares
};

static int enc_plan(gam_handle* h, int B, int64_t T, int n_layers_run, const int64_t* feat_len_host, EncPlan& p) {
  const gam_config& c = h->cfg;
  if (B <= 0 || T <= 0) return fail(h, -1, "bad shape B=%d T=%lld", B, (long long)T);
  p.B = B; p.T = T;
  p.D = c.d_model; p.F = c.feat_in; p.H = c.n_heads; p.dk = p.D / p.H; p.DFF = p.D * c.ff_expansion_factor;
  p.T1 = (int)half_up(T); p.Tv = (int)half_up(p.T1);
  if (p.Tv > c.pos_emb_max_len) return fail(h, -1, "%d encoder frames exceed pos_emb_max_len %d", p.Tv, c.pos_emb_max_len);
  if (p.Tv <= 0) return fail(h, -1, "no encoder frames");
  p.conv2d = c.subsampling == GAM_SUBS_CONV2D;
  p.rel = c.self_attention_model == GAM_ATT_REL_POS;
  p.nl = n_layers_run < 0 ? c.n_layers : std::min(n_layers_run, c.n_layers);
  // Ta: per-utterance row stride of every token-major buffer (>= T' ; the extra rows are
  // treated as padding).  conv2d: image rows per utterance = 2*Ta >= T1 + 2.
  // conv1d: stage-1 output rows per utterance = 2*Ta >= T1 + 4.
  p.Ta = p.conv2d ? std::max(p.Tv + 1, (p.T1 + 3) / 2) : std::max(p.Tv, (p.T1 + 5) / 2);
  p.N = B * p.Ta;
  // conv1d: stage-1 input rows per utterance: 2*T1a >= T + 2*pad ; stage-1 output = stage-2 input rows: 2*Ta
  const int pad = (c.subs_kernel_size - 1) / 2;
  p.T1a = p.conv2d ? 0 : std::max(p.T1, (int)((T + 2 * pad + 1) / 2));
  // Packed rows (gam_pack.h): with the lengths known on the HOST (gam_encode_varlen) a ragged batch runs its layers on the valid frames
  // only -- NR rows instead of N, utterance b at rows cu[b] .. -- when that drops at least 3 % of the rows.  Equal-length batches, single
  // utterances and callers without host lengths keep the padded layout (and its results, bit for bit).
  p.packed = false;
  p.NR = p.N; p.Tmax = p.Ta;
  // (below graph_max_rows the step is launch-bound and replayed as a hipGraph keyed on the padded shape: fewer rows buy nothing there and a
  //  row count in the key would defeat the replay -- packed rows start where the graph regime ends; GAM_PACK=2 forces them at any size: tests)
  const bool pack_regime = h->use_pack >= 2 || !h->use_graph || p.N >= h->graph_max_rows;
  if (feat_len_host != nullptr && h->use_pack && pack_regime && B > 1 && B <= 1024) {
    long long sum = 0;
    int mx = 0;
    for (int b = 0; b < B; ++b) {
      const int64_t l = std::min<int64_t>(std::max<int64_t>(feat_len_host[b], 0), T);
      const int l2 = (int)half_up(half_up(l));      // = len2 of gam_lengths_kernel
      sum += l2;
      mx = std::max(mx, l2);
    }
    if (sum > 0 && sum * 100 <= (long long)p.N * 97) { p.packed = true; p.NR = (int)sum; p.Tmax = mx; }
  }
  // Split-fp16 modes: every encoder GEMM runs on the LDS-DMA kernel of gam_gemm_sp.h, and the kernels that
  // produce its A operands (LayerNorm, SiLU epilogue, attention, conv module, stem) write them in the
  // sp32 split layout instead of fp32 -- same bytes, no conversion pass.
  p.sp = split_mode(h) && p.D % 32 == 0 && p.DFF % 32 == 0;
  // operand format the producers write (gam_common.h gam_store4).  Format 2 (plain fp16, GAM_GEMM_F16) packs 64 k-values into
  // the 128-byte line of a k-tile, so every reduction length / row pitch must be a multiple of 64; a model whose d_model or
  // FFN width is 32 x an odd number keeps the three-term kernels for its GEMMs in that mode (as gam_op_gemm does)
  // instead of failing half-way through a batch with the stem image already written as fp16.
  const bool f16_fmt_ok = p.D % 64 == 0 && p.DFF % 64 == 0;   // (the stem's channel count is D)
  p.spf = p.sp ? (h->gemm_mode == GAM_GEMM_F16 && f16_fmt_ok ? 2 : 1) : 0;
  // conv1d stem: both GEMMs read overlapping rows (lda = 2F / 2C < K).  In the split modes xin and y1 hold sp32 (a row starts on a
  // 32-element block of the flat buffer, F % 32 == 0), and both GEMMs are three-term in the one-term mode too.
  p.sp_stem = p.sp && p.F % 32 == 0;
  // Small batches: the layer sequence is replayed as one hipGraph (see gam_handle::use_graph).  (packed rows: the row count is part of
  // every launch)
  p.graph = h->use_graph && !h->prof_on && p.nl > 0 && p.N < h->graph_max_rows && !p.packed;
  return 0;
}

// Everything the call touches exists behind this function: the stem, the layers and a capture allocate nothing.
static int enc_workspace(gam_handle* h, const EncPlan& p, EncBufs& w) {
  const size_t B = p.B, N = p.N, D = p.D, Ta = p.Ta;
  if (int r = ensure(h, h->lens, 4 * B)) return r;
  const size_t maxB = h->lens.cap / 4;
  w.len0 = h->lens.as<int>(); w.len1 = w.len0 + maxB; w.len2 = w.len0 + 2 * maxB; w.elen = w.len0 + 3 * maxB;
  if (int r = ensure(h, h->x, N * D)) return r;
  if (int r = ensure(h, h->y, N * D)) return r;
  if (int r = ensure(h, h->yr, N * D)) return r;
  if (int r = ensure(h, h->hbuf, N * p.DFF)) return r;
  if (int r = ensure(h, h->qkv, N * 3 * D)) return r;
  if (int r = ensure(h, h->ctx, N * D)) return r;
  if (int r = ensure(h, h->ubuf, N * 2 * D)) return r;
  if (int r = ensure(h, h->zbuf, N * D)) return r;
  if (int r = ensure(h, h->rsbuf, N + 64)) return r;
  if (p.packed)
    if (int r = ensure(h, h->pack_idx, (size_t)1032 + 2 * N)) return r;
  w.cu = p.packed ? reinterpret_cast<int*>(h->pack_idx.p) : nullptr;
  w.row_t = p.packed ? w.cu + 1032 : nullptr;
  w.row_src = p.packed ? w.row_t + N : nullptr;
  // sp32 operands: every LayerNorm hands its GEMMs a per-row power-of-two scale (gam_row_scale; the exact-fp32 kernel undoes none)
  w.rs = p.sp && h->use_rowscale ? h->rsbuf.p : nullptr;
  if (p.conv2d) {   // the zero-bordered image (+ two slack rows) and Conv2d#2's output
    if (int r = ensure(h, h->img, (B * 2 * Ta + 2) * (h->f1 + 1) * D)) return r;
    if (int r = ensure(h, h->c2, N * h->f2 * D)) return r;
  } else {
    if (int r = ensure(h, h->xin, (B * 2 * p.T1a + 8) * p.F)) return r;
    if (int r = ensure(h, h->y1, (B * 2 * Ta + 8) * D)) return r;
  }
  if (p.rel)
    if (int r = ensure(h, h->pbuf, (size_t)(2 * p.Tv - 1) * D)) return r;
  if (p.graph)   // the largest split-K partial sums of a layer GEMM: a capture may not allocate
    if (int r = ensure(h, h->splitk_ws, (size_t)16 * N * std::max(p.DFF, 2 * p.D) + 64)) return r;
  return 0;
}

static GamLnArgs enc_ln_args(const gam_handle* h, const EncPlan& p, const EncBufs& w) {
  GamLnArgs ln;
  memset(&ln, 0, sizeof ln);
  ln.rows = p.NR; ln.d = p.D; ln.ta = p.Ta; ln.row_t = w.row_t; ln.dk = p.dk; ln.eps = 1e-5f; ln.rcos = h->rot_cos; ln.rsin = h->rot_sin;
  ln.rope_rows = h->cfg.pos_emb_max_len;
  ln.rs = w.rs;
  return ln;
}

static int enc_lengths(gam_handle* h, hipStream_t s, const EncPlan& p, const EncBufs& w, const int64_t* feat_len) {
  ProfScope ps(h, s, GAM_PF_MISC, 0.0);
  hipLaunchKernelGGL(gam_lengths_kernel, dim3(gam_cdiv(p.B, 64)), dim3(64), 0, s, (const long long*)feat_len, p.B, (int)p.T, 2,
                     w.len0, w.len1, w.len2, w.elen);
  HIPCHK(h, hipGetLastError());
  if (p.packed) {
    hipLaunchKernelGGL(gam_pack_index_kernel, dim3(1), dim3(256), 0, s, w.len2, p.B, p.Ta, p.NR, w.cu, w.row_t, w.row_src, h->range_flag);
    HIPCHK(h, hipGetLastError());
  }
  return 0;
}

// The operand formats of one encoder GEMM: A as sp32 in format a_fmt (0: A stays fp32) with its per-row scale, C's store format and
// the range guard on C.
static inline void gemm_formats(GamGemmArgs& g, int a_fmt, const float* a_rs, int c_split, int c_guard) {
  if (a_fmt) { g.Asp = reinterpret_cast<const _Float16*>(g.A); g.a_fmt = a_fmt; }
  g.a_rs = a_rs; g.c_split = c_split; g.c_guard = c_guard;
}

// ------------------------------ stem ------------------------------
// (C == D, and sp already implies D % 32 == 0: the image and both GEMMs' operands are sp32 whenever sp is set)
static int stem_conv2d(gam_handle* h, hipStream_t s, const EncPlan& p, const EncBufs& w, const float* feat) {
  const int B = p.B, Ta = p.Ta, N = p.N, C = p.D, D = p.D, FP = h->f1 + 1, F2 = h->f2;
  {
    GamConv1Args a;
    a.feat = feat; a.img = h->img.p; a.w = h->c1_w; a.bias = h->c1_b; a.len0 = w.len0; a.len1 = w.len1;
    a.B = B; a.T = (int)p.T; a.F = p.F; a.Ta = Ta; a.FP = FP; a.C = C; a.T1 = p.T1;
    a.img_split = p.spf;
    a.range_flag = h->use_range ? h->range_flag : nullptr;
    ProfScope ps(h, s, GAM_PF_STEM, (double)B * 2 * Ta * FP * C * 4.0);
    if (a.img_split == 2) hipLaunchKernelGGL(gam_conv2d1_kernel<2>, dim3(2 * Ta, B), dim3(256), 0, s, a);
    else if (a.img_split == 1) hipLaunchKernelGGL(gam_conv2d1_kernel<1>, dim3(2 * Ta, B), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(gam_conv2d1_kernel<0>, dim3(2 * Ta, B), dim3(256), 0, s, a);
    HIPCHK(h, hipGetLastError());
    // two slack rows past the last utterance (read by its padding frame only); the dense fp16 image ends at half the offset
    const size_t img_end = (size_t)B * 2 * Ta * FP * C;
    HIPCHK(h, hipMemsetAsync(a.img_split == 2 ? reinterpret_cast<float*>(reinterpret_cast<_Float16*>(h->img.p) + img_end) : h->img.p + img_end, 0,
                             (size_t)2 * FP * C * sizeof(float), s));
  }
  GamGemmArgs g = gemm_args(h->img.p, 0, h->c2_w, h->c2_b, h->c2.p, C, N * F2, C, 9 * C);
  g.a_mode = 1; g.conv_fp = FP; g.conv_c = C; g.conv_f2 = F2;
  g.lens = w.len2; g.rpb = Ta * F2; g.fdiv = F2;
  g.skip_pad = p.packed ? 1 : 0;      // 16-frame row tiles behind an utterance's last frame: 12 rounds of tiles shrink with the batch's padding
  gemm_formats(g, p.spf, nullptr, p.spf, 1);
  if (int r = gemm(h, s, g, GAM_ACT_RELU, GAM_PF_CONV2, &h->s_c2)) return r;
  GamGemmArgs l = gemm_args(h->c2.p, (long)F2 * C, h->lin_w, h->lin_b, p.packed ? h->y.p : h->x.p, D, N, D, F2 * C);
  gemm_formats(l, p.spf, nullptr, 0, 0);
  return gemm(h, s, l, GAM_ACT_NONE, GAM_PF_GEMM, &h->s_lin);
}

static int stem_conv1d(gam_handle* h, hipStream_t s, const EncPlan& p, const EncBufs& w, const float* feat) {
  const int B = p.B, Ta = p.Ta, T1a = p.T1a, N = p.N, C = p.D, D = p.D, F = p.F;
  const int64_t T = p.T;
  const int ks = h->cfg.subs_kernel_size, pad = (ks - 1) / 2;
  const int fmt = p.sp_stem ? 1 : 0;   // (all-zero bits are an sp32 zero: the memsets serve both formats)
  {
    ProfScope ps(h, s, GAM_PF_STEM, (double)B * T * F * 8.0);
    HIPCHK(h, hipMemsetAsync(h->xin.p, 0, ((size_t)B * 2 * T1a + 8) * F * sizeof(float), s));
    HIPCHK(h, hipMemsetAsync(h->y1.p, 0, ((size_t)B * 2 * Ta + 8) * C * sizeof(float), s));
    dim3 grid(gam_cdiv(T, 32), gam_cdiv(F, 32), B);
    int* const rf = h->use_range ? h->range_flag : nullptr;
    if (p.sp_stem) hipLaunchKernelGGL(gam_feat_to_rows_kernel<1>, grid, dim3(256), 0, s, feat, h->xin.p, w.len0, B, F, (int)T, 2 * T1a, pad, rf);
    else hipLaunchKernelGGL(gam_feat_to_rows_kernel<0>, grid, dim3(256), 0, s, feat, h->xin.p, w.len0, B, F, (int)T, 2 * T1a, pad, rf);
    HIPCHK(h, hipGetLastError());
  }
  GamGemmArgs g1 = gemm_args(h->xin.p, 2L * F, h->c1_w, h->c1_b, h->y1.p, C, B * T1a, C, ks * F);
  g1.lens = w.len1; g1.rpb = T1a; g1.fdiv = 1;
  g1.remap = 1; g1.out_rpb = 2 * Ta; g1.out_shift = pad; g1.rows_valid = std::min(T1a, 2 * Ta - pad);
  gemm_formats(g1, fmt, nullptr, fmt, 1);
  if (int r = gemm(h, s, g1, GAM_ACT_RELU, GAM_PF_CONV2, &h->s_c1)) return r;
  GamGemmArgs g2 = gemm_args(h->y1.p, 2L * C, h->c2_w, h->c2_b, p.packed ? h->y.p : h->x.p, D, N, D, ks * C);
  g2.lens = w.len2; g2.rpb = Ta; g2.fdiv = 1;
  gemm_formats(g2, fmt, nullptr, 0, 0);
  return gemm(h, s, g2, GAM_ACT_RELU, GAM_PF_CONV2, &h->s_c2);
}

static int enc_stem(gam_handle* h, hipStream_t s, const EncPlan& p, const EncBufs& w, const float* feat) {
  if (int r = p.conv2d ? stem_conv2d(h, s, p, w, feat) : stem_conv1d(h, s, p, w, feat)) return r;
  if (p.packed) {   // the stem's padded rows -> packed rows (the only copy the layout costs: 2 x NR x D x 4 bytes)
    ProfScope ps(h, s, GAM_PF_STEM, (double)p.NR * p.D * 8.0);
    hipLaunchKernelGGL(gam_gather_rows_kernel, dim3(std::min(4096, gam_cdiv(p.NR * (p.D / 4), 256))), dim3(256), 0, s, h->y.p, w.row_src, h->x.p, p.NR, p.D);
    HIPCHK(h, hipGetLastError());
  }
  return 0;
}

// ------------------------------ Conformer layers ------------------------------
// One builder and launcher per non-GEMM kernel family, shared by the layer blocks and the gam_op_* entry points (which make
// their own argument checks and open no ProfScope).  dk is GAM_ATT_DK for every handle (gam_create).
static int launch_attention(gam_handle* h, hipStream_t s, const float* q, const float* k, const float* v, long ldq, float* ctx, int ctx_split,
                            const int* lens, const int* cu, int B, int Ta, int Tv, int H, const float* pbuf, const float* pos_u,
                            const float* pos_v) {
  const int D = H * GAM_ATT_DK;
  GamAttnArgs at;
  memset(&at, 0, sizeof at);
  at.q = q; at.k = k; at.v = v; at.ctx = ctx; at.ctx_split = ctx_split; at.lens = lens; at.cu = cu;
  at.B = B; at.Ta = Ta; at.Tv = Tv; at.H = H; at.ldq = ldq; at.ldv = ldq; at.ldo = D;
  at.scale = 1.0f / sqrtf((float)GAM_ATT_DK);
  at.pbuf = pbuf; at.pos_u = pos_u; at.pos_v = pos_v; at.ldp = D;
  hipError_t e = gam_launch_attn_mode(at, GAM_ATT_DK, split_mode(h), s, h->gemm_mode == GAM_GEMM_F16 ? 1 : 3, h->ncu);
  if (e != hipSuccess) return fail(h, -2, "attention launch: %s", hipGetErrorString(e));
  return 0;
}

// (returns the launch's error: the encoder and gam_op_convmod word their failures differently)
static hipError_t launch_convmod(gam_handle* h, hipStream_t s, const float* u, float* z, const float* dw_w, const float* dw_b, const float* n_scale,
                                 const float* n_shift, const int* lens, const int* cu, int B, int Ta, int Tv, int d, int ks, bool layer_norm,
                                 int z_split) {
  GamConvModArgs cm;
  memset(&cm, 0, sizeof cm);
  cm.u = u; cm.z = z; cm.dw_w = dw_w; cm.dw_b = dw_b; cm.n_scale = n_scale; cm.n_shift = n_shift;
  cm.lens = lens; cm.cu = cu; cm.B = B; cm.Ta = Ta; cm.Tv = Tv; cm.d = d; cm.ks = ks; cm.eps = 1e-5f;
  cm.z_split = z_split; cm.range_flag = h->use_range ? h->range_flag : nullptr;
  return gam_launch_convmod(cm, layer_norm, s);
}

// LayerNorm of x into the GEMM operand y
static int norm_to_y(gam_handle* h, hipStream_t s, const EncCtx& c, const float* w, const float* b, PendingReduce* pend) {
  GamLnArgs a = c.ln;
  a.x = h->x.p; a.out1 = h->y.p; a.w1 = w; a.b1 = b;
  a.split1 = c.p.spf;
  return layernorm(h, s, a, 0, pend);
}

// x += 0.5 * W2 silu(W1 y + b1) + b2, y = the LayerNorm of x (already applied)
static int ffn_block(gam_handle* h, hipStream_t s, const EncCtx& c, const float* w1, const float* b1, const W16& s_w1, const float* w2,
                     const float* b2, const W16& s_w2, PendingReduce* pend) {
  const int D = c.p.D, DFF = c.p.DFF, NR = c.p.NR, spf = c.p.spf;
  GamGemmArgs g = gemm_args(h->y.p, D, w1, b1, h->hbuf.p, DFF, NR, DFF, D);
  gemm_formats(g, spf, c.w.rs, spf, 1);
  if (int r = gemm(h, s, g, GAM_ACT_SILU, GAM_PF_GEMM, &s_w1)) return r;
  GamGemmArgs g2 = gemm_args(h->hbuf.p, DFF, w2, b2, h->x.p, D, NR, D, DFF);
  g2.R = h->x.p; g2.ldr = D; g2.alpha = 0.5f;
  gemm_formats(g2, spf, nullptr, 0, 0);
  return gemm(h, s, g2, GAM_ACT_NONE, GAM_PF_GEMM, &s_w2, pend);
}

static int attn_block(gam_handle* h, hipStream_t s, const EncCtx& c, const LayerW& L, PendingReduce* pend) {
  const EncPlan& p = c.p;
  const int D = p.D, NR = p.NR, Tv = p.Tv, spf = p.spf;
  float* const rs = c.w.rs;
  GamLnArgs a = c.ln;
  a.x = h->x.p; a.out1 = h->y.p; a.out2 = h->yr.p; a.w1 = L.ln_att_w; a.b1 = L.ln_att_b;
  a.split1 = spf; a.split2 = spf;
  if (int r = layernorm(h, s, a, p.rel ? 0 : 1, pend)) return r;
  // rotary: q,k project the rotated copy, v the plain one; rel_pos: all three project y.  One [N, 3D] result q | k | v.
  // q, k and v are split to fp16 unscaled by the attention kernel: range guard on all of them.
  const bool one_launch = p.rel || (p.sp && (2 * D) % 256 == 0);   // (the operand switch sits on a tile boundary of either tile width)
  if (one_launch) {
    GamGemmArgs gq = gemm_args(p.rel ? h->y.p : h->yr.p, D, L.wqkv, L.bqkv, h->qkv.p, 3 * D, NR, 3 * D, D);
    gemm_formats(gq, spf, rs, 0, 1);
    if (!p.rel) { gq.Asp2 = reinterpret_cast<const _Float16*>(h->y.p); gq.n_switch = 2 * D; }
    if (int r = gemm(h, s, gq, GAM_ACT_NONE, GAM_PF_GEMM, &L.s_wqkv)) return r;
  } else {
    GamGemmArgs gq = gemm_args(h->yr.p, D, L.wqkv, L.bqkv, h->qkv.p, 3 * D, NR, 2 * D, D);
    gemm_formats(gq, spf, rs, 0, 1);
    if (int r = gemm(h, s, gq, GAM_ACT_NONE, GAM_PF_GEMM, &L.s_wqkv)) return r;
    W16 wv16 = L.s_wqkv;   // rows 2D .. 3D of the same planes
    const size_t off = (size_t)2 * D * D;
    wv16.h16 += off;
    if (wv16.sp) wv16.sp += 2 * off;
    GamGemmArgs gv = gemm_args(h->y.p, D, L.wqkv + off, L.bqkv + 2 * D, h->qkv.p + 2 * D, 3 * D, NR, D, D);
    gemm_formats(gv, spf, rs, 0, 1);
    if (int r = gemm(h, s, gv, GAM_ACT_NONE, GAM_PF_GEMM, &wv16)) return r;
  }
  if (p.rel) {  // P = linear_pos(pos_emb) for relative positions -(T'-1) .. T'-1 (no bias)
    const size_t pe0 = (size_t)(h->cfg.pos_emb_max_len - 1 - (Tv - 1)) * D;
    GamGemmArgs gp = gemm_args(h->rel_pe + pe0, D, L.wpos, nullptr, h->pbuf.p, D, 2 * Tv - 1, D, D);
    if (p.sp) { gp.Asp = reinterpret_cast<const _Float16*>(h->rel_pe_sp + pe0); gp.a_fmt = 1; }   // (three-term in the one-term mode too)
    if (int r = gemm(h, s, gp, GAM_ACT_NONE, GAM_PF_GEMM, &L.s_wpos)) return r;
  }
  {
    ProfScope ps(h, s, GAM_PF_ATTN, 4.0 * (double)p.B * p.H * (double)Tv * Tv * p.dk);
    // (encoder.py:620-624: no mask at batch 1)
    if (int r = launch_attention(h, s, h->qkv.p, h->qkv.p + D, h->qkv.p + 2 * D, 3 * D, h->ctx.p, spf, p.B > 1 ? c.w.len2 : nullptr, c.w.cu, p.B,
                                 p.packed ? p.Tmax : p.Ta, Tv, p.H, p.rel ? h->pbuf.p : nullptr, L.pos_u, L.pos_v))
      return r;
  }
  GamGemmArgs go = gemm_args(h->ctx.p, D, L.wo, L.bo, h->x.p, D, NR, D, D);
  go.R = h->x.p; go.ldr = D;
  gemm_formats(go, spf, nullptr, 0, 0);
  return gemm(h, s, go, GAM_ACT_NONE, GAM_PF_GEMM, &L.s_wo, pend);
}

static int conv_block(gam_handle* h, hipStream_t s, const EncCtx& c, const LayerW& L, PendingReduce* pend) {
  const EncPlan& p = c.p;
  const int D = p.D, NR = p.NR, ks = h->cfg.conv_kernel_size;
  if (int r = norm_to_y(h, s, c, L.ln_conv_w, L.ln_conv_b, pend)) return r;
  GamGemmArgs g1 = gemm_args(h->y.p, D, L.pw1_w, L.pw1_b, h->ubuf.p, 2 * D, NR, 2 * D, D);
  gemm_formats(g1, p.spf, c.w.rs, 0, 0);
  if (int r = gemm(h, s, g1, GAM_ACT_NONE, GAM_PF_GEMM, &L.s_pw1)) return r;
  {
    ProfScope ps(h, s, GAM_PF_CONVMOD, (double)NR * D * 3 * 4.0);
    hipError_t e = launch_convmod(h, s, h->ubuf.p, h->zbuf.p, L.dw_w, L.dw_b, L.cn_scale, L.cn_shift, c.w.len2, c.w.cu, p.B,
                                  p.packed ? p.Tmax : p.Ta, p.Tv, D, ks, h->cfg.conv_norm_type == GAM_NORM_LAYER, p.spf);
    if (e != hipSuccess) return fail(h, -2, "conv-module launch (k=%d): %s", ks, hipGetErrorString(e));
  }
  GamGemmArgs g2 = gemm_args(h->zbuf.p, D, L.pw2_w, L.pw2_b, h->x.p, D, NR, D, D);
  g2.R = h->x.p; g2.ldr = D;
  gemm_formats(g2, p.spf, nullptr, 0, 0);
  return gemm(h, s, g2, GAM_ACT_NONE, GAM_PF_GEMM, &L.s_pw2, pend);
}

// norm_out in place, fused with the next layer's norm_feed_forward1 into y when there is one
static int norm_out_block(gam_handle* h, hipStream_t s, const EncCtx& c, const LayerW& L, const LayerW* next, PendingReduce* pend) {
  GamLnArgs a = c.ln;
  a.x = h->x.p; a.out1 = h->x.p; a.w1 = L.ln_out_w; a.b1 = L.ln_out_b;
  if (next != nullptr) {
    a.out2 = h->y.p; a.w2 = next->ln_ff1_w; a.b2 = next->ln_ff1_b;
    a.split2 = c.p.spf;
    return layernorm(h, s, a, 2, pend);
  }
  a.rs = nullptr;   // the last norm_out feeds no GEMM
  return layernorm(h, s, a, 0, pend);
}

static int run_layers(gam_handle* h, hipStream_t s, const EncCtx& c) {
  const int nl = c.p.nl;
  if (nl > 0)
    if (int r = norm_to_y(h, s, c, h->layers[0].ln_ff1_w, h->layers[0].ln_ff1_b, nullptr)) return r;
  PendingReduce pend;    // the split-K slices of the residual GEMM just launched, summed by the LayerNorm that follows it
  for (int li = 0; li < nl; ++li) {
    const LayerW& L = h->layers[li];
    if (int r = ffn_block(h, s, c, L.ff1_w1, L.ff1_b1, L.s_ff1_w1, L.ff1_w2, L.ff1_b2, L.s_ff1_w2, &pend)) return r;   // macaron half step
    if (int r = attn_block(h, s, c, L, &pend)) return r;
    if (int r = conv_block(h, s, c, L, &pend)) return r;
    if (int r = norm_to_y(h, s, c, L.ln_ff2_w, L.ln_ff2_b, &pend)) return r;
    if (int r = ffn_block(h, s, c, L.ff2_w1, L.ff2_b1, L.s_ff2_w1, L.ff2_w2, L.ff2_b2, L.s_ff2_w2, &pend)) return r;
    if (int r = norm_out_block(h, s, c, L, li + 1 < nl ? &h->layers[li + 1] : nullptr, &pend)) return r;
  }
  return flush_pending(h, s, &pend);   // (nothing is pending after a norm_out; kept so that a future reordering cannot lose a reduce)
}

// Small batches: replay the layer sequence as one hipGraph (see gam_handle::use_graph).  *replayed = the layers ran from a graph;
// otherwise the caller launches them.
static int replay_layers(gam_handle* h, hipStream_t s, const EncCtx& c, bool* replayed) {
  typedef gam_handle::GraphEntry Entry;
  const EncPlan& p = c.p;
  *replayed = false;
  if (!p.graph) return 0;
  const GamSpForce& frc = gam_sp_force();   // (a plan forced through gam_tune_sp after a capture must not replay the old tiling)
  const std::vector<int> key = {p.B, p.Ta, p.Tv, p.nl, h->gemm_mode, (int)p.sp, h->use_splitk, h->fuse_reduce, frc.mt.load(), frc.nw.load(), frc.s.load(), frc.ns.load()};
  Entry& ge = h->graphs[key];
  if (ge.gen != h->ws_generation) {   // a buffer moved since this entry was made
    if (ge.exec) { hipGraphExecDestroy(ge.exec); --h->graph_count; }
    ge = Entry();
    ge.gen = h->ws_generation;
  }
  if (ge.exec == nullptr && ge.seen == Entry::SEEN_ONCE && h->graph_count >= 32) ge.seen = Entry::PLAIN_ONLY;   // cache full: plain launches
  if (ge.exec == nullptr && ge.seen == Entry::SEEN_ONCE) {
    hipGraph_t graph = nullptr;
    if (h->cap_stream == nullptr && hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking) != hipSuccess)
      h->cap_stream = nullptr;
    if (h->cap_stream != nullptr && hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeRelaxed) == hipSuccess) {
      const int r = run_layers(h, h->cap_stream, c);     // recorded, not executed
      const hipError_t e = hipStreamEndCapture(h->cap_stream, &graph);
      if (r == 0 && e == hipSuccess && graph != nullptr && h->ws_generation == ge.gen &&
          hipGraphInstantiate(&ge.exec, graph, nullptr, nullptr, 0) != hipSuccess)
        ge.exec = nullptr;
      if (graph) hipGraphDestroy(graph);
    }
    (void)hipGetLastError();               // a refused capture must not poison the launches below
    if (ge.exec == nullptr) { ge.seen = Entry::PLAIN_ONLY; ++h->graph_captures_failed; }   // capture failed: never try this shape again
    else ++h->graph_count;
  }
  if (ge.exec != nullptr) {
    HIPCHK(h, hipGraphLaunch(ge.exec, s));
    *replayed = true;
    ++h->graph_replays;
  } else if (ge.seen == Entry::UNSEEN) {
    ge.seen = Entry::SEEN_ONCE;
  }
  return 0;
}

// ------------------------------ outputs ------------------------------
// channel-first `encoded`, token-major `tokens_out` and `enc_len`, each optional, from padded or packed rows
static int enc_outputs(gam_handle* h, hipStream_t s, const EncPlan& p, const EncBufs& w, float* encoded, float* tokens_out, int32_t* enc_len) {
  const int B = p.B, Ta = p.Ta, Tv = p.Tv, D = p.D;
  ProfScope ps(h, s, GAM_PF_MISC, (double)B * Tv * D * 8.0);
  if (encoded && p.packed) {
    hipLaunchKernelGGL(gam_unpack_transpose_kernel, dim3(gam_cdiv(D, 32), gam_cdiv(Tv, 32), B), dim3(256), 0, s, h->x.p, w.cu, w.len2, encoded, Tv, D);
    HIPCHK(h, hipGetLastError());
  } else if (encoded) {
    hipError_t e = gam_launch_transpose(h->x.p, encoded, B, Tv, D, (size_t)Ta * D, D, (size_t)D * Tv, Tv, s);
    if (e != hipSuccess) return fail(h, -2, "transpose launch: %s", hipGetErrorString(e));
  }
  if (tokens_out && p.packed) {
    hipLaunchKernelGGL(gam_unpack_rows_kernel, dim3(std::min(4096, gam_cdiv(B * Tv * (D / 4), 256))), dim3(256), 0, s, h->x.p, w.cu, w.len2, tokens_out, B, Tv, D);
    HIPCHK(h, hipGetLastError());
  } else if (tokens_out)
    HIPCHK(h, hipMemcpy2DAsync(tokens_out, (size_t)Tv * D * 4, h->x.p, (size_t)Ta * D * 4, (size_t)Tv * D * 4, B, hipMemcpyDeviceToDevice, s));
  if (enc_len) HIPCHK(h, hipMemcpyAsync(enc_len, w.elen, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, s));
  return 0;
}

static int encode_impl(gam_handle* h, const float* feat, const int64_t* feat_len, int B, int64_t T, float* encoded,
                       int32_t* enc_len, int n_layers_run, float* tokens_out, hipStream_t s, const int64_t* feat_len_host = nullptr) {
  if (!h || !h->finalized) return fail(h, -1, "gam_encode before gam_finalize");
  if (!h->has_encoder) return fail(h, -1, "this handle was finalized without encoder weights");
  EncCtx c;
  if (int r = enc_plan(h, B, T, n_layers_run, feat_len_host, c.p)) return r;
  HIPCHK(h, hipSetDevice(h->device));
  h->last_rows = c.p.NR;
  h->last_rows_padded = c.p.N;
  if (int r = enc_workspace(h, c.p, c.w)) return r;
  c.ln = enc_ln_args(h, c.p, c.w);
  if (int r = enc_lengths(h, s, c.p, c.w, feat_len)) return r;
  if (int r = enc_stem(h, s, c.p, c.w, feat)) return r;
  bool replayed = false;
  if (int r = replay_layers(h, s, c, &replayed)) return r;
  if (!replayed)
    if (int r = run_layers(h, s, c)) return r;
  return enc_outputs(h, s, c.p, c.w, encoded, tokens_out, enc_len);
}

int gam_encode(gam_handle* h, const float* feat, const int64_t* feat_len, int B, int64_t T, float* encoded, int32_t* enc_len,
               void* stream) {
  return encode_impl(h, feat, feat_len, B, T, encoded, enc_len, -1, nullptr, (hipStream_t)stream);
}

int gam_encode_ex(gam_handle* h, const float* feat, const int64_t* feat_len, int B, int64_t T, float* encoded, int32_t* enc_len,
                  int n_layers_run, float* tokens_out, void* stream) {
  return encode_impl(h, feat, feat_len, B, T, encoded, enc_len, n_layers_run, tokens_out, (hipStream_t)stream);
}

int gam_encode_varlen(gam_handle* h, const float* feat, const int64_t* feat_len, const int64_t* feat_len_host, int B, int64_t T,
                      float* encoded, int32_t* enc_len, int n_layers_run, float* tokens_out, void* stream) {
  return encode_impl(h, feat, feat_len, B, T, encoded, enc_len, n_layers_run, tokens_out, (hipStream_t)stream, feat_len_host);
}

// -----------------------------------------------------------------------------------
// heads: encoded [B,D,Tp] -> token-major [B*Tp, D] once, then GEMMs
static int to_tokens(gam_handle* h, const float* encoded, int B, int64_t Tp, hipStream_t s) {
  const int D = h->cfg.d_model;
  if (int r = ensure(h, h->tok, (size_t)B * Tp * D)) return r;
  ProfScope ps(h, s, GAM_PF_DECODE, (double)B * Tp * D * 8.0);
  hipError_t e = gam_launch_transpose(encoded, h->tok.p, B, D, (int)Tp, (size_t)D * Tp, Tp, (size_t)Tp * D, D, s);
  if (e != hipSuccess) return fail(h, -2, "transpose launch: %s", hipGetErrorString(e));
  return 0;
}

// The CTC head's logits [B * Tp, V] into h->logits.  The caller has made the head check (head_check).
static int ctc_logits(gam_handle* h, const float* encoded, int B, int64_t Tp, hipStream_t s) {
  if (B <= 0 || Tp <= 0) return fail(h, -1, "bad shape B=%d T'=%lld", B, (long long)Tp);
  HIPCHK(h, hipSetDevice(h->device));
  const int D = h->cfg.d_model, V = h->cfg.num_classes;
  if (int r = to_tokens(h, encoded, B, Tp, s)) return r;
  if (int r = ensure(h, h->logits, (size_t)B * Tp * V)) return r;
  GamGemmArgs g = gemm_args(h->tok.p, D, h->ctc_w, h->ctc_b, h->logits.p, V, (int)(B * Tp), V, D);
  return gemm(h, s, g, GAM_ACT_NONE, GAM_PF_DECODE);
}

// The encoder half of the RNN-T joint for a whole batch: encoded [B, D, Tp] -> [B * Tp, JH] = W_enc f + b_enc, into h->encp or, when
// given, into the caller's `out` (gam_rnnt_encp).
static int rnnt_encp(gam_handle* h, const float* encoded, int B, int64_t Tp, hipStream_t s, float* out = nullptr) {
  const int D = h->cfg.d_model, JH = h->cfg.joint_hidden;
  if (int r = to_tokens(h, encoded, B, Tp, s)) return r;
  if (!out)
    if (int r = ensure(h, h->encp, (size_t)B * Tp * JH)) return r;
  GamGemmArgs g = gemm_args(h->tok.p, D, h->jn_enc_w, h->jn_enc_b, out ? out : h->encp.p, JH, (int)(B * Tp), JH, D);
  return gemm(h, s, g, GAM_ACT_NONE, GAM_PF_DECODE);
}

// The CTC head's log-probs [B * Tp, V]: the logits GEMM into h->logits, then the log-softmax into `out` -- NULL: in place on h->logits
// (each row is read whole by its wave before that wave writes it).
static int ctc_log_probs(gam_handle* h, const float* encoded, int B, int64_t Tp, float* out, hipStream_t s) {
  if (int r = ctc_logits(h, encoded, B, Tp, s)) return r;
  const int V = h->cfg.num_classes, rows = (int)(B * Tp);
  ProfScope ps(h, s, GAM_PF_DECODE, (double)rows * V * 8.0);
  hipLaunchKernelGGL(gam_log_softmax_kernel, dim3(gam_cdiv(rows, 4)), dim3(256), 0, s, h->logits.p, out ? out : h->logits.p, rows, V);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int gam_ctc_head(gam_handle* h, const float* encoded, int B, int64_t Tp, float* log_probs, void* stream) {
  if (int r = head_check(h, GAM_HEAD_CTC, "CTC head")) return r;
  GAM_DECODE_ENTRY(h, stream);
  return ctc_log_probs(h, encoded, B, Tp, log_probs, s);
}

int gam_ctc_greedy(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, int32_t* ids,
                   int32_t* frames, int32_t* counts, void* stream) {
  if (int r = head_check(h, GAM_HEAD_CTC, "CTC head")) return r;
  GAM_DECODE_ENTRY(h, stream);
  if (int r = ctc_logits(h, encoded, B, Tp, s)) return r;
  const int V = h->cfg.num_classes;
  const size_t sm = ((size_t)Tp + GAM_CTC_NT / 64 + 8) * sizeof(int);
  if (sm > 60 * 1024) return fail(h, -1, "T'=%lld too long for the CTC greedy kernel", (long long)Tp);
  ProfScope ps(h, s, GAM_PF_DECODE, (double)B * Tp * V * 4.0);
  hipLaunchKernelGGL(gam_ctc_greedy_kernel, dim3(B), dim3(GAM_CTC_NT), sm, s, h->logits.p, enc_len, (int)Tp, V, ids, frames, counts);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// CTC forced alignment over log-probs [B, Tp, V] (gam_align.h): one workgroup per utterance.  Decode class (the caller holds a DecodeScope):
// the backpointer scratch is the handle's.  star != NULL: the STAR variant of the kernel (target id V is the wildcard, emission star [B, Tp]).
static int ctc_align_launch(gam_handle* h, const float* lp, const int32_t* enc_len, int B, int64_t Tp, int V, const int32_t* targets,
                            const int32_t* target_len, int Umax, int32_t* frame_labels, int32_t* tok_first, int32_t* tok_last,
                            float* score, float* loglik, int32_t* status, hipStream_t s, const float* star = nullptr) {
  if (B <= 0 || Tp <= 0 || V < 2) return fail(h, -1, "CTC alignment: bad shape B=%d T'=%lld V=%d", B, (long long)Tp, V);
  if (Tp > GAM_ALIGN_MAX_T) return fail(h, -1, "CTC alignment: T'=%lld frames exceed the limit %d", (long long)Tp, GAM_ALIGN_MAX_T);
  if (Umax < 0 || Umax > GAM_ALIGN_MAX_U) return fail(h, -1, "CTC alignment: Umax=%d tokens outside [0, %d]", Umax, GAM_ALIGN_MAX_U);
  if (!lp || !enc_len || !target_len || !frame_labels || !score || !loglik || !status ||
      (Umax > 0 && (!targets || !tok_first || !tok_last)))
    return fail(h, -1, "CTC alignment: NULL buffer");
  const int smax = 2 * Umax + 1;
  const int nt = std::min(GAM_ALIGN_MAX_NT, std::max(64, (smax + 63) / 64 * 64));
  const int spt = (smax + nt - 1) / nt;
  const int nchunk = (smax + 63) / 64;
  const bool bp_lds = gam_align_lds_bytes(true, (int)Tp, nchunk, spt, nt) <= GAM_ALIGN_LDS_MAX;
  const size_t sm = gam_align_lds_bytes(bp_lds, (int)Tp, nchunk, spt, nt);
  if (sm > GAM_ALIGN_LDS_MAX) return fail(h, -1, "CTC alignment: T'=%lld x Umax=%d needs %zu bytes of LDS", (long long)Tp, Umax, sm);
  GamAlignStarArgs a;          // (the plain kernels take its GamAlignArgs base)
  a.star = star;
  a.lp = lp; a.enc_len = enc_len; a.targets = targets; a.target_len = target_len;
  a.Tp = (int)Tp; a.V = V; a.Umax = Umax; a.nchunk = nchunk; a.bp_glob = nullptr;
  a.frame_labels = frame_labels; a.tok_first = tok_first; a.tok_last = tok_last; a.score = score; a.loglik = loglik; a.status = status;
  if (!bp_lds) {
    if (int r = ensure(h, h->align_bp, (size_t)B * Tp * nchunk * 4 + 64)) return r;
    a.bp_glob = reinterpret_cast<uint4*>(h->align_bp.p);
  }
  static std::atomic<unsigned long long> lds_set[12];
  const int which = (bp_lds ? 3 : 0) + (spt - 1);
  void (*const kerns[6])(GamAlignArgs) = {gam_ctc_align_kernel<false, 1>, gam_ctc_align_kernel<false, 2>, gam_ctc_align_kernel<false, 3>,
                                          gam_ctc_align_kernel<true, 1>, gam_ctc_align_kernel<true, 2>, gam_ctc_align_kernel<true, 3>};
  void (*const skerns[6])(GamAlignStarArgs) = {
      gam_ctc_align_kernel<false, 1, GamAlignStarArgs>, gam_ctc_align_kernel<false, 2, GamAlignStarArgs>,
      gam_ctc_align_kernel<false, 3, GamAlignStarArgs>, gam_ctc_align_kernel<true, 1, GamAlignStarArgs>,
      gam_ctc_align_kernel<true, 2, GamAlignStarArgs>,  gam_ctc_align_kernel<true, 3, GamAlignStarArgs>};
  if (sm > 64 * 1024)
    HIPCHK(h, gam_set_max_lds(star ? (const void*)skerns[which] : (const void*)kerns[which], GAM_ALIGN_LDS_MAX, lds_set[(star ? 6 : 0) + which]));
  ProfScope ps(h, s, GAM_PF_DECODE, (double)B * Tp * smax * 4.0);
  if (star) hipLaunchKernelGGL(skerns[which], dim3(B), dim3(nt), sm, s, a);
  else hipLaunchKernelGGL(kerns[which], dim3(B), dim3(nt), sm, s, static_cast<const GamAlignArgs&>(a));
  HIPCHK(h, hipGetLastError());
  return 0;
}

int gam_ctc_align(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, const int32_t* targets,
                  const int32_t* target_len, int Umax, int32_t* frame_labels, int32_t* tok_first, int32_t* tok_last, float* score,
                  float* loglik, int32_t* status, void* stream) {
  if (int r = head_check(h, GAM_HEAD_CTC, "CTC head")) return r;
  GAM_DECODE_ENTRY(h, stream);
  if (Tp > GAM_ALIGN_MAX_T || Umax < 0 || Umax > GAM_ALIGN_MAX_U)
    return fail(h, -1, "CTC alignment: T'=%lld / Umax=%d beyond the limits (%d / %d)", (long long)Tp, Umax, GAM_ALIGN_MAX_T, GAM_ALIGN_MAX_U);
  if (int r = ctc_log_probs(h, encoded, B, Tp, nullptr, s)) return r;
  const int V = h->cfg.num_classes;
  return ctc_align_launch(h, h->logits.p, enc_len, B, Tp, V, targets, target_len, Umax, frame_labels, tok_first, tok_last, score,
                          loglik, status, s);
}

int gam_op_ctc_align(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, const int32_t* targets,
                     const int32_t* target_len, int Umax, int32_t* frame_labels, int32_t* tok_first, int32_t* tok_last, float* score,
                     float* loglik, int32_t* status, void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  return ctc_align_launch(h, log_probs, enc_len, B, Tp, V, targets, target_len, Umax, frame_labels, tok_first, tok_last, score, loglik,
                          status, s);
}

// ---- wildcard tokens (target id V; gam_trellis.h).  Additions: the entry points above keep rejecting id V.
static int ctc_star_penalty_check(gam_handle* h, float penalty) {
  if (!std::isfinite(penalty) || penalty < 0.f) return fail(h, -1, "CTC wildcard: penalty %g must be finite and >= 0", (double)penalty);
  return 0;
}

// star[row] = max_v lp[row, v] - penalty over rows = B * Tp (enc_len NULL: every row is valid)
static int ctc_star_row_launch(gam_handle* h, const float* lp, const int32_t* enc_len, int B, int64_t Tp, int V, float penalty, float* star,
                               hipStream_t s) {
  const long rows = (long)B * Tp;
  if (rows == 0) return 0;
  ProfScope ps(h, s, GAM_PF_DECODE, (double)rows * V * 4.0);
  hipLaunchKernelGGL(gam_ctc_star_row_kernel, dim3(gam_cdiv(rows, 4)), dim3(256), 0, s, lp, enc_len, (int)Tp, V, rows, penalty, star);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int gam_op_ctc_star_row(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, float penalty,
                        float* star_lp, void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  if (B <= 0 || Tp < 0 || V < 2 || (int64_t)B * Tp > 2147483647ll * 4)
    return fail(h, -1, "CTC wildcard row: bad shape B=%d T'=%lld V=%d", B, (long long)Tp, V);
  if (int r = ctc_star_penalty_check(h, penalty)) return r;
  if (Tp > 0 && (!log_probs || !star_lp)) return fail(h, -1, "CTC wildcard row: NULL buffer");
  return ctc_star_row_launch(h, log_probs, enc_len, B, Tp, V, penalty, star_lp, s);
}

int gam_ctc_align_star(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, const int32_t* targets,
                       const int32_t* target_len, int Umax, float penalty, int32_t* frame_labels, int32_t* tok_first, int32_t* tok_last,
                       float* score, float* loglik, int32_t* status, void* stream) {
  if (int r = head_check(h, GAM_HEAD_CTC, "CTC head")) return r;
  GAM_DECODE_ENTRY(h, stream);
  if (Tp > GAM_ALIGN_MAX_T || Umax < 0 || Umax > GAM_ALIGN_MAX_U)
    return fail(h, -1, "CTC alignment: T'=%lld / Umax=%d beyond the limits (%d / %d)", (long long)Tp, Umax, GAM_ALIGN_MAX_T, GAM_ALIGN_MAX_U);
  if (int r = ctc_star_penalty_check(h, penalty)) return r;
  if (!enc_len) return fail(h, -1, "CTC alignment: NULL buffer");
  if (int r = ctc_log_probs(h, encoded, B, Tp, nullptr, s)) return r;
  const int V = h->cfg.num_classes;
  if (int r = ensure(h, h->align_star, (size_t)B * Tp + 64)) return r;
  if (int r = ctc_star_row_launch(h, h->logits.p, enc_len, B, Tp, V, penalty, h->align_star.p, s)) return r;
  return ctc_align_launch(h, h->logits.p, enc_len, B, Tp, V, targets, target_len, Umax, frame_labels, tok_first, tok_last, score,
                          loglik, status, s, h->align_star.p);
}

int gam_op_ctc_align_star(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, const float* star_lp,
                          const int32_t* targets, const int32_t* target_len, int Umax, int32_t* frame_labels, int32_t* tok_first,
                          int32_t* tok_last, float* score, float* loglik, int32_t* status, void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  if (!star_lp) return fail(h, -1, "CTC alignment: NULL buffer");
  return ctc_align_launch(h, log_probs, enc_len, B, Tp, V, targets, target_len, Umax, frame_labels, tok_first, tok_last, score, loglik,
                          status, s, star_lp);
}

// CTC forced alignment of ONE long utterance (gam_align_long.h): the anti-diagonal sweep launches, the backtrack and the outputs kernel on
// one stream.  Decode class: the workspace is the handle's.  wild: the STAR variants of the prep and sweep kernels, emissions star [T].
static int ctc_align_long_launch(gam_handle* h, const float* log_probs, int64_t T, int V, bool wild, const float* star, const int32_t* targets, int U,
                                 int32_t* frame_labels, int32_t* tok_first, int32_t* tok_last, double* score, double* loglik,
                                 int32_t* status, hipStream_t s) {
  if (T < 0 || T > 2147483647ll || V < 2 || U < 0 || U > (1 << 30) - 1)
    return fail(h, -1, "long CTC alignment: bad shape T=%lld V=%d U=%d", (long long)T, V, U);
  if (!score || !loglik || !status || (T > 0 && (!log_probs || !frame_labels)) || (U > 0 && (!targets || !tok_first || !tok_last)))
    return fail(h, -1, "long CTC alignment: NULL buffer");
  const GamAlignLongForce& frc = gam_align_long_force();
  const int fsb = frc.sb.load(), ftt = frc.tt.load();
  GamAlignLongStarArgs a;      // (the plain kernels take its GamAlignLongArgs base)
  a.star = star;
  a.lp = log_probs; a.targets = targets; a.T = (int)T; a.V = V; a.U = U;
  a.sb = fsb ? fsb : GAM_AL_SB_DEFAULT;
  a.tt = ftt ? ftt : GAM_AL_TT_DEFAULT;
  const int64_t S = 2 * (int64_t)U + 1;
  a.nS = (int)((S + a.sb - 1) / a.sb);
  a.nT = (int)((T + a.tt - 1) / a.tt);
  a.nchunk = (int)((S + 63) / 64);
  a.frame_labels = frame_labels; a.tok_first = tok_first; a.tok_last = tok_last; a.score = score; a.loglik = loglik; a.status = status;
  // workspace, every part 256-byte aligned: backpointers | edges | rows d, a | offsets | path | ctrl
  auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
  const size_t n_bp = up((size_t)T * a.nchunk * 16), n_edge = up((size_t)a.nS * T * 16), n_row = up((size_t)a.nS * a.sb * 4);
  const size_t n_off = up((size_t)a.nS * 16), n_path = up((size_t)T * 4), n_ctrl = 256;
  const size_t need = n_bp + n_edge + 2 * n_row + n_off + n_path + n_ctrl;
  if (need > h->al_ws_limit)
    return fail(h, -1, "long CTC alignment: T=%lld x U=%d needs %zu bytes of workspace, the limit is %zu bytes (gam_set_ctc_align_workspace / "
                "GAM_CTC_ALIGN_WS)", (long long)T, U, need, h->al_ws_limit);
  if (int r = ensure(h, h->align_long_ws, need / 4)) return r;
  unsigned char* w = reinterpret_cast<unsigned char*>(h->align_long_ws.p);
  a.bp = reinterpret_cast<uint4*>(w); w += n_bp;
  a.edge = reinterpret_cast<double2*>(w); w += n_edge;
  a.rowD = reinterpret_cast<float*>(w); w += n_row;
  a.rowA = reinterpret_cast<float*>(w); w += n_row;
  a.off = reinterpret_cast<double2*>(w); w += n_off;
  a.path = reinterpret_cast<int*>(w); w += n_path;
  a.ctrl = reinterpret_cast<int*>(w);
  int nt = 0, spt = 0;
  gam_align_long_shape(a.sb, &nt, &spt);
  const size_t sm = gam_align_long_lds_bytes(spt, nt);
  HIPCHK(h, hipMemsetAsync(a.ctrl, 0, 16, s));
  const GamAlignLongArgs& a0 = a;
  if (U > 0) {
    if (wild) hipLaunchKernelGGL(gam_ctc_align_long_prep_kernel<true>, dim3(gam_cdiv(U, 256)), dim3(256), 0, s, a0);
    else hipLaunchKernelGGL(gam_ctc_align_long_prep_kernel<false>, dim3(gam_cdiv(U, 256)), dim3(256), 0, s, a0);
  }
  if (T > 0 && T >= U) {      // (T < U is infeasible whatever the ids are: the outputs kernel alone reports it)
    ProfScope ps(h, s, GAM_PF_DECODE, (double)T * (double)S * 4.0);
    for (int d = 0; d < a.nT + a.nS - 1; ++d) {
      const int jlo = std::max(0, d - (a.nT - 1)), jhi = std::min(a.nS - 1, d);
      const dim3 grid(jhi - jlo + 1);
      if (wild) {
        if (spt == 1) hipLaunchKernelGGL((gam_ctc_align_long_sweep_kernel<1, GamAlignLongStarArgs>), grid, dim3(nt), sm, s, a, d);
        else if (spt == 2) hipLaunchKernelGGL((gam_ctc_align_long_sweep_kernel<2, GamAlignLongStarArgs>), grid, dim3(nt), sm, s, a, d);
        else hipLaunchKernelGGL((gam_ctc_align_long_sweep_kernel<3, GamAlignLongStarArgs>), grid, dim3(nt), sm, s, a, d);
      } else if (spt == 1) hipLaunchKernelGGL(gam_ctc_align_long_sweep_kernel<1>, grid, dim3(nt), sm, s, a0, d);
      else if (spt == 2) hipLaunchKernelGGL(gam_ctc_align_long_sweep_kernel<2>, grid, dim3(nt), sm, s, a0, d);
      else hipLaunchKernelGGL(gam_ctc_align_long_sweep_kernel<3>, grid, dim3(nt), sm, s, a0, d);
    }
  }
  if (T > 0 && T >= U) {
    ProfScope ps(h, s, GAM_PF_ALIGN_BT, (double)T * 16.0);
    hipLaunchKernelGGL(gam_ctc_align_long_backtrack_kernel, dim3(1), dim3(64), 0, s, a0);
  }
  const int64_t n_out = std::max<int64_t>(std::max<int64_t>(T, U), 1);
  ProfScope ps(h, s, GAM_PF_ALIGN_OUT, (double)T * 8.0 + (double)U * 8.0);
  hipLaunchKernelGGL(gam_ctc_align_long_outputs_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, a0);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int gam_op_ctc_align_long(gam_handle* h, const float* log_probs, int64_t T, int V, const int32_t* targets, int U, int32_t* frame_labels,
                          int32_t* tok_first, int32_t* tok_last, double* score, double* loglik, int32_t* status, void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  return ctc_align_long_launch(h, log_probs, T, V, false, nullptr, targets, U, frame_labels, tok_first, tok_last, score, loglik, status, s);
}

int gam_op_ctc_align_long_star(gam_handle* h, const float* log_probs, int64_t T, int V, const float* star_lp, const int32_t* targets, int U,
                               int32_t* frame_labels, int32_t* tok_first, int32_t* tok_last, double* score, double* loglik,
                               int32_t* status, void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  if (T > 0 && !star_lp) return fail(h, -1, "long CTC alignment: NULL buffer");
  return ctc_align_long_launch(h, log_probs, T, V, true, star_lp, targets, U, frame_labels, tok_first, tok_last, score, loglik,
                               status, s);
}

// Windowed longform (gam_stitch.h).  Decode class both; neither synchronises with the host.
int gam_op_ctc_stitch(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, const int32_t* lo,
                      const int32_t* hi, const int64_t* dst, float* out, int64_t T_total, int32_t* status, void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  if (B < 1 || B > 65535 || Tp < 1 || Tp > 2147483647ll || V < 1 || T_total < 0)
    return fail(h, -1, "CTC stitch: bad shape B=%d T'=%lld V=%d T_total=%lld", B, (long long)Tp, V, (long long)T_total);
  if (!log_probs || !enc_len || !lo || !hi || !dst || !status || (T_total > 0 && !out)) return fail(h, -1, "CTC stitch: NULL buffer");
  GamStitchArgs a;
  a.lp = log_probs; a.enc_len = enc_len; a.lo = lo; a.hi = hi; a.dst = reinterpret_cast<const long long*>(dst); a.out = out; a.status = status;
  a.Tp = Tp; a.T_total = T_total; a.V = V;
  // 16 floats per thread and pass at the widest access; the grid stride covers whatever the cap leaves over
  const int64_t chunks = std::min<int64_t>(std::max<int64_t>((Tp * V + 4095) / 4096, 1), 4096);
  ProfScope ps(h, s, GAM_PF_DECODE, (double)B * Tp * V * 8.0);
  hipLaunchKernelGGL(gam_ctc_stitch_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(256), 0, s, a);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int gam_op_ctc_greedy_long(gam_handle* h, const float* log_probs, int64_t T, int V, int32_t* ids, int32_t* frames, int32_t* count,
                           void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  if (T < 0 || T > 2147483647ll || V < 2 || V > GAM_BEAM_MAX_V)
    return fail(h, -1, "long CTC greedy decode: bad shape T=%lld V=%d (2 <= V <= %d)", (long long)T, V, GAM_BEAM_MAX_V);
  if (!count || (T > 0 && (!log_probs || !ids || !frames))) return fail(h, -1, "long CTC greedy decode: NULL buffer");
  const bool per_thread = V <= 64 && (V & 1) == 0;      // the two argmax forms of gam_ctc_greedy_kernel
  const int fb = per_thread ? GAM_GL_FB : GAM_GL_FBW;
  const int nblk = (int)((T + fb - 1) / fb);
  if (int r = ensure(h, h->greedy_long_ws, (size_t)T + (size_t)nblk + 64)) return r;
  int* lab = h->greedy_long_ws.as<int>();
  int* blk = lab + T;
  ProfScope ps(h, s, GAM_PF_DECODE, (double)T * V * 4.0);
  if (nblk > 0) {
    if (per_thread) hipLaunchKernelGGL(gam_ctc_greedy_long_labels_kernel<GAM_GL_FB>, dim3(nblk), dim3(GAM_GL_FB), 0, s, log_probs, (long long)T, V, lab, blk);
    else hipLaunchKernelGGL(gam_ctc_greedy_long_labels_kernel<GAM_GL_FBW>, dim3(nblk), dim3(GAM_GL_FB), 0, s, log_probs, (long long)T, V, lab, blk);
  }
  hipLaunchKernelGGL(gam_ctc_greedy_long_scan_kernel, dim3(1), dim3(GAM_GL_SCAN_NT), 0, s, blk, nblk, count);
  if (nblk > 0) {
    if (per_thread) hipLaunchKernelGGL(gam_ctc_greedy_long_compact_kernel<GAM_GL_FB>, dim3(nblk), dim3(GAM_GL_FB), 0, s, lab, blk, (long long)T, ids, frames);
    else hipLaunchKernelGGL(gam_ctc_greedy_long_compact_kernel<GAM_GL_FBW>, dim3(nblk), dim3(GAM_GL_FBW), 0, s, lab, blk, (long long)T, ids, frames);
  }
  HIPCHK(h, hipGetLastError());
  return 0;
}

int gam_set_ctc_align_workspace(gam_handle* h, int64_t bytes) {
  if (!h) return -1;
  if (bytes < 0) return fail(h, -1, "long CTC alignment: workspace limit %lld bytes is negative", (long long)bytes);
  h->al_ws_limit = bytes == 0 ? GAM_AL_WS_DEFAULT : (size_t)bytes;
  return 0;
}

int gam_tune_ctc_align_long(int sb, int tt) {
  // (multiples of 64 only: whole backpointer chunks, and EVEN -- the one-edge-state scheme of gam_align_long.h rests on it)
  if (sb != 0 && (sb < 64 || sb > GAM_AL_SB_MAX || sb % 64 != 0)) return -1;
  if (tt < 0) return -1;
  GamAlignLongForce& f = gam_align_long_force();
  f.sb = sb; f.tt = tt;
  return 0;
}

// ---- keyword search (gam_kws.h).  Decode class (the caller holds a DecodeScope): the row-maximum workspace is the handle's.
int gam_set_keywords(gam_handle* h, const int32_t* tokens, const int32_t* offsets, int n_keywords, const float* min_score) {
  if (!h) return -1;
  if (n_keywords < 0 || n_keywords > GAM_KWS_MAX_K)
    return fail(h, -1, "keywords: %d keywords outside [0, %d]", n_keywords, GAM_KWS_MAX_K);
  if (n_keywords > 0 && (!tokens || !offsets || !min_score)) return fail(h, -1, "keywords: NULL buffer");
  int max_tok = -1, ntok = 0;
  if (n_keywords > 0) {
    if (offsets[0] != 0) return fail(h, -1, "keywords: offsets[0] = %d, expected 0", offsets[0]);
    // (a handle without a CTC head learns V with the log-probs: gam_op_ctc_kws checks the ids then)
    const int hi = h->cfg.head_type == GAM_HEAD_CTC && h->cfg.num_classes >= 2 ? h->cfg.num_classes - 2 : 0x3fffffff;
    for (int i = 0; i < n_keywords; ++i) {
      const int a = offsets[i], e = offsets[i + 1];
      if (e <= a) return fail(h, -1, "keywords: keyword %d is empty or its offsets decrease", i);
      if (e - a > GAM_KWS_MAX_U) return fail(h, -1, "keywords: keyword %d has %d tokens, the limit is %d", i, e - a, GAM_KWS_MAX_U);
      if (!std::isfinite(min_score[i]) || min_score[i] > 0.f)
        return fail(h, -1, "keywords: min_score[%d] = %g must be finite and <= 0", i, (double)min_score[i]);
      for (int k = a; k < e; ++k) {
        const int c = tokens[k];
        if (c < 0 || c > hi) return fail(h, -1, "keywords: token id %d of keyword %d outside [0, %d]", c, i, hi);
        max_tok = std::max(max_tok, c);
      }
    }
    ntok = offsets[n_keywords];
  }
  HIPCHK(h, hipSetDevice(h->device));
  // a decode-class kernel still in flight may read the current set
  if (h->dec_evt != nullptr && h->dec_evt_set) HIPCHK(h, hipEventSynchronize(h->dec_evt));
  ++h->kw_gen;
  if (n_keywords == 0) {
    h->kw_K = h->kw_ntok = 0;
    h->kw_max_tok = -1;
    HIPCHK(h, h->kw_dev.release());
    return 0;
  }
  std::vector<int> flat((size_t)n_keywords + 1 + ntok + n_keywords);
  memcpy(flat.data(), offsets, ((size_t)n_keywords + 1) * sizeof(int));
  memcpy(flat.data() + n_keywords + 1, tokens, (size_t)ntok * sizeof(int));
  memcpy(flat.data() + n_keywords + 1 + ntok, min_score, (size_t)n_keywords * sizeof(float));
  if (int r = ensure_table(h, h->kw_dev, flat.size())) return r;
  HIPCHK(h, hipMemcpy(h->kw_dev.p, flat.data(), flat.size() * sizeof(int), hipMemcpyHostToDevice));
  h->kw_K = n_keywords;
  h->kw_ntok = ntok;
  h->kw_max_tok = max_tok;
  return 0;
}

// Everything the two entry points check before a launch (shape, limits, the keyword set against V).
static int ctc_kws_check(gam_handle* h, int B, int64_t Tp, int V, int max_hits, bool null_buf) {
  if (B <= 0 || Tp <= 0 || V < 2) return fail(h, -1, "keyword search: bad shape B=%d T'=%lld V=%d", B, (long long)Tp, V);
  if (Tp > GAM_KWS_MAX_T) return fail(h, -1, "keyword search: T'=%lld frames exceed the limit %d", (long long)Tp, GAM_KWS_MAX_T);
  if (max_hits < 1 || max_hits > GAM_KWS_MAX_HITS)
    return fail(h, -1, "keyword search: max_hits=%d outside [1, %d]", max_hits, GAM_KWS_MAX_HITS);
  if (!h->kw_dev.p || h->kw_K <= 0) return fail(h, -1, "keyword search: no keyword set (gam_set_keywords)");
  if (h->kw_max_tok > V - 2) return fail(h, -1, "keyword search: keyword token id %d outside [0, %d] for V=%d", h->kw_max_tok, V - 2, V);
  if ((int64_t)B * ((h->kw_K + GAM_KWS_WAVES - 1) / GAM_KWS_WAVES) > 2147483647ll)
    return fail(h, -1, "keyword search: B=%d x %d keywords exceed the grid", B, h->kw_K);
  if (null_buf) return fail(h, -1, "keyword search: NULL buffer");
  return 0;
}

// The row-maximum pre-pass and the search kernel over log-probs [B, Tp, V] (the checks are the caller's).
static int ctc_kws_launch(gam_handle* h, const float* lp, const int32_t* enc_len, int B, int64_t Tp, int V, int max_hits,
                          int32_t* hit_frames, float* hit_score, int32_t* n_hits, float* dense_score, int32_t* dense_start,
                          hipStream_t s) {
  const long rows = (long)B * Tp;
  if (int r = ensure(h, h->kws_mb, (size_t)rows * 2 + 64)) return r;
  {
    ProfScope ps(h, s, GAM_PF_DECODE, (double)rows * V * 4.0);
    hipLaunchKernelGGL(gam_kws_rowmax_kernel, dim3(gam_cdiv(rows, 4)), dim3(256), 0, s, lp, enc_len, (int)Tp, V, rows,
                       reinterpret_cast<float2*>(h->kws_mb.p));
    HIPCHK(h, hipGetLastError());
  }
  const int K = h->kw_K;
  GamKwsArgs a;
  a.lp = lp; a.enc_len = enc_len; a.mb = reinterpret_cast<const float2*>(h->kws_mb.p);
  a.kw_off = h->kw_dev.as<int>(); a.kw_tok = a.kw_off + K + 1; a.kw_min = reinterpret_cast<const float*>(a.kw_tok + h->kw_ntok);
  a.B = B; a.Tp = (int)Tp; a.V = V; a.K = K; a.max_hits = max_hits;
  a.hit_frames = hit_frames; a.hit_score = hit_score; a.n_hits = n_hits; a.dense_score = dense_score; a.dense_start = dense_start;
  ProfScope ps(h, s, GAM_PF_DECODE, (double)rows * K * 64.0 * 4.0);
  const dim3 grid(B * gam_cdiv(K, GAM_KWS_WAVES)), block(64 * GAM_KWS_WAVES);
  if (dense_score || dense_start) hipLaunchKernelGGL(gam_ctc_kws_kernel<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(gam_ctc_kws_kernel<false>, grid, block, 0, s, a);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int gam_ctc_kws(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, int max_hits, int32_t* hit_frames,
                float* hit_score, int32_t* n_hits, float* dense_score, int32_t* dense_start, void* stream) {
  if (int r = head_check(h, GAM_HEAD_CTC, "CTC head")) return r;
  GAM_DECODE_ENTRY(h, stream);
  const int V = h->cfg.num_classes;
  if (int r = ctc_kws_check(h, B, Tp, V, max_hits, !encoded || !enc_len || !hit_frames || !hit_score || !n_hits)) return r;
  if (int r = ctc_log_probs(h, encoded, B, Tp, nullptr, s)) return r;
  return ctc_kws_launch(h, h->logits.p, enc_len, B, Tp, V, max_hits, hit_frames, hit_score, n_hits, dense_score, dense_start, s);
}

int gam_op_ctc_kws(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, int max_hits,
                   int32_t* hit_frames, float* hit_score, int32_t* n_hits, float* dense_score, int32_t* dense_start, void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  if (int r = ctc_kws_check(h, B, Tp, V, max_hits, !log_probs || !enc_len || !hit_frames || !hit_score || !n_hits)) return r;
  return ctc_kws_launch(h, log_probs, enc_len, B, Tp, V, max_hits, hit_frames, hit_score, n_hits, dense_score, dense_start, s);
}

// ---- the same search for one stream fed in pieces (gam_kws.h gam_ctc_kws_stream_kernel).  Decode class as above.
int64_t gam_ctc_kws_state_bytes(gam_handle* h) {
  if (!h) return -1;
  if (!h->kw_dev.p || h->kw_K <= 0) return fail(h, -1, "keyword search: no keyword set (gam_set_keywords)");
  return (int64_t)h->kw_K * GAM_KWS_ST_WORDS * 4;
}

int gam_op_ctc_kws_stream(gam_handle* h, const float* log_probs, int64_t n, int V, int64_t t_base, int flags, void* state, int max_hits,
                          int32_t* hit_frames, float* hit_score, int32_t* n_hits, int32_t* status, float* dense_score,
                          int32_t* dense_start, void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  if (n < 0 || t_base < 0 || V < 2 || n >= 2147483648ll || t_base >= 2147483648ll || t_base + n >= 2147483648ll)
    return fail(h, -1, "keyword stream: bad shape n=%lld V=%d t_base=%lld (t_base + n must stay below 2^31)", (long long)n, V,
                (long long)t_base);
  if (flags & ~(GAM_KWS_F_BEGIN | GAM_KWS_F_END)) return fail(h, -1, "keyword stream: unknown flags 0x%x", flags);
  if (max_hits < 1 || max_hits > GAM_KWS_STREAM_MAX_HITS)
    return fail(h, -1, "keyword stream: max_hits=%d outside [1, %d]", max_hits, GAM_KWS_STREAM_MAX_HITS);
  if (!h->kw_dev.p || h->kw_K <= 0) return fail(h, -1, "keyword search: no keyword set (gam_set_keywords)");
  if (h->kw_max_tok > V - 2) return fail(h, -1, "keyword search: keyword token id %d outside [0, %d] for V=%d", h->kw_max_tok, V - 2, V);
  // (n < 2^31 rows are n / 4 < 2^29 workgroups of the row-maximum pass, and n x V < 2^62 is indexed in 64 bits: no further limit)
  if ((n > 0 && !log_probs) || !state || !hit_frames || !hit_score || !n_hits || !status) return fail(h, -1, "keyword stream: NULL buffer");
  if (n > 0) {
    if (int r = ensure(h, h->kws_mb, (size_t)n * 2 + 64)) return r;
    ProfScope ps(h, s, GAM_PF_DECODE, (double)n * V * 4.0);
    hipLaunchKernelGGL(gam_kws_rowmax_kernel, dim3(gam_cdiv(n, 4)), dim3(256), 0, s, log_probs, (const int*)nullptr, (int)n, V, (long)n,
                       reinterpret_cast<float2*>(h->kws_mb.p));
    HIPCHK(h, hipGetLastError());
  }
  const int K = h->kw_K;
  GamKwsStreamArgs a;
  a.lp = log_probs; a.mb = reinterpret_cast<const float2*>(h->kws_mb.p);
  a.kw_off = h->kw_dev.as<int>(); a.kw_tok = a.kw_off + K + 1; a.kw_min = reinterpret_cast<const float*>(a.kw_tok + h->kw_ntok);
  a.n = (int)n; a.V = V; a.K = K; a.max_hits = max_hits; a.t_base = (int)t_base; a.flags = flags; a.gen = h->kw_gen;
  a.state = static_cast<int*>(state); a.hit_frames = hit_frames; a.hit_score = hit_score; a.n_hits = n_hits; a.status = status;
  a.dense_score = dense_score; a.dense_start = dense_start;
  ProfScope ps(h, s, GAM_PF_DECODE, (double)n * K * 64.0 * 4.0);
  const dim3 grid(gam_cdiv(K, GAM_KWS_WAVES)), block(64 * GAM_KWS_WAVES);
  if (dense_score || dense_start) hipLaunchKernelGGL(gam_ctc_kws_stream_kernel<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(gam_ctc_kws_stream_kernel<false>, grid, block, 0, s, a);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// ---- what the two beam searches share (gam_search.h): the handle's hotwords and LM as kernel arguments, the common checks, the launch
static GamHwArgs hw_args(const gam_handle* h, bool hw_lds) {
  GamHwArgs a;
  a.trie = h->hw_trie.as<int>(); a.nodes = h->hw_nodes; a.words = h->hw_words; a.lds = hw_lds ? 1 : 0; a.beta = h->hw_boost;
  return a;
}
static GamLmArgs lm_args(const gam_handle* h) {
  GamLmArgs a;
  a.lm_cls = h->lm_cls.as<int>();
  a.lm_wt = h->lm_wt.as<const uint4>();
  a.lm_ng = h->lm_ng.as<const uint4>();
  a.lm_wmask = h->lm_wslots - 1; a.lm_wprobe = h->lm_wprobe; a.lm_nmask = h->lm_nslots - 1; a.lm_nprobe = h->lm_nprobe;
  a.lm_m = h->lm_order - 1; a.lm_bos = h->lm_bos; a.lm_eos = h->lm_eos; a.lm_unk = h->lm_unk;
  a.lm_unk_logp = h->lm_unk_logp; a.lm_alpha = h->lm_alpha; a.lm_beta = h->lm_beta;
  return a;
}
// Width, buffers, and the handle's hotwords and LM against V.  `name` opens the messages; `lm_fmt` is the search's own LM message
// (the LM's V, the search's V).
static int beam_check(gam_handle* h, const char* name, int W, int V, bool null_buffer, const char* lm_fmt) {
  if (W < 1 || W > GAM_BEAM_MAX_W) return fail(h, -1, "%s: beam width W=%d outside [1, %d]", name, W, GAM_BEAM_MAX_W);
  if (null_buffer) return fail(h, -1, "%s: NULL buffer", name);
  if (h->hw_trie.p && h->hw_max_tok > V - 2)
    return fail(h, -1, "%s: hotword token id %d outside [0, %d] for V=%d", name, h->hw_max_tok, V - 2, V);
  if (h->lm_ng.p && h->lm_V != V) return fail(h, -1, lm_fmt, h->lm_V, V);
  return 0;
}
// The N-best calls' own check (n_hyp != NULL marks an N-best call): 1 <= N <= W <= 32.
static int nbest_check(gam_handle* h, const char* name, int W, int N, const int32_t* n_hyp) {
  if (N < 1 || N > W || N > GAM_BEAM_MAX_W) return fail(h, -1, "%s: N=%d hypotheses outside [1, min(W, %d)] for W=%d", name, N, GAM_BEAM_MAX_W, W);
  if (!n_hyp) return fail(h, -1, "%s: NULL buffer", name);
  return 0;
}
// Launch one instantiation of a beam kernel; its LDS limit is raised once (`once`: one word per instantiation) when it needs > 64 KiB.
static int beam_launch(gam_handle* h, const void* kern, std::atomic<unsigned long long>& once, size_t max_lds, int B, int nt, size_t sm,
                       hipStream_t s, void* args) {
  if (max_lds > 64 * 1024) HIPCHK(h, gam_set_max_lds(kern, (int)max_lds, once));
  HIPCHK(h, hipLaunchKernel(kern, dim3(B), dim3(nt), &args, sm, s));
  return 0;
}

// CTC prefix beam search over log-probs [B, Tp, V] (gam_beam.h): one workgroup per utterance.  Decode class (the caller holds a
// DecodeScope): the prefix-trie nodes are the handle's.  nbest: the <.., true> kernels, ids / frames [B, N, Tp] and counts / score / logp
// [B, N]; else N and n_hyp are not read.
static int ctc_beam_launch(gam_handle* h, const float* lp, const int32_t* enc_len, int B, int64_t Tp, int V, int W, int32_t* ids,
                           int32_t* frames, int32_t* counts, float* score, float* logp, hipStream_t s, bool nbest = false, int N = 0,
                           int32_t* n_hyp = nullptr) {
  if (B <= 0 || Tp <= 0 || V < 2 || V > GAM_BEAM_MAX_V) return fail(h, -1, "CTC beam search: bad shape B=%d T'=%lld V=%d", B, (long long)Tp, V);
  if (Tp > GAM_ALIGN_MAX_T) return fail(h, -1, "CTC beam search: T'=%lld frames exceed the limit %d", (long long)Tp, GAM_ALIGN_MAX_T);
  if (int r = beam_check(h, "CTC beam search", W, V, !lp || !enc_len || !ids || !frames || !counts || !score || !logp,
                         "CTC beam search: the LM's token classes are for V=%d, the log-probs have V=%d"))
    return r;
  if (nbest)
    if (int r = nbest_check(h, "CTC beam search", W, N, n_hyp)) return r;
  const int K = std::min(W, V - 1);
  const bool lm = h->lm_ng.p != nullptr;
  const bool hw_lds = h->hw_trie.p && (size_t)h->hw_words * 4 <= GAM_BEAM_HW_LDS_MAX;
  const size_t sm = gam_beam_lds_bytes(W, K, V, hw_lds ? h->hw_words : 0, lm);
  if (int r = ensure(h, h->beam_nodes, (size_t)B * Tp * W * 2 + 64)) return r;
  GamBeamArgs a;
  a.lp = lp; a.enc_len = enc_len; a.Tp = (int)Tp; a.V = V; a.W = W; a.K = K;
  a.hw = hw_args(h, hw_lds);
  a.lm = lm_args(h);
  a.nodes = reinterpret_cast<int2*>(h->beam_nodes.p);
  a.ids = ids; a.frames = frames; a.counts = counts; a.score = score; a.logp = logp;
  a.nb.n_hyp = nbest ? n_hyp : nullptr; a.nb.n = nbest ? N : 0; a.nb.pad = 0;
  static std::atomic<unsigned long long> lds_set[4];
  static const void* const kern[4] = {(const void*)gam_ctc_beam_kernel<false, false>, (const void*)gam_ctc_beam_kernel<true, false>,
                                      (const void*)gam_ctc_beam_kernel<false, true>, (const void*)gam_ctc_beam_kernel<true, true>};
  const int ki = (lm ? 1 : 0) + (nbest ? 2 : 0);
  ProfScope ps(h, s, GAM_PF_DECODE, (double)B * Tp * W * (K + 1) * 4.0);
  return beam_launch(h, kern[ki], lds_set[ki], sm, B, GAM_BEAM_NT, sm, s, &a);
}

// gam_ctc_beam / gam_ctc_beam_nbest: the CTC head, its log-softmax in place, the beam kernel.
static int ctc_beam_run(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, int W, int32_t* ids, int32_t* frames,
                        int32_t* counts, float* score, float* logp, void* stream, bool nbest, int N, int32_t* n_hyp) {
  if (int r = head_check(h, GAM_HEAD_CTC, "CTC head")) return r;
  GAM_DECODE_ENTRY(h, stream);
  if (Tp > GAM_ALIGN_MAX_T || W < 1 || W > GAM_BEAM_MAX_W)
    return fail(h, -1, "CTC beam search: T'=%lld / W=%d beyond the limits (%d / [1, %d])", (long long)Tp, W, GAM_ALIGN_MAX_T, GAM_BEAM_MAX_W);
  if (nbest)
    if (int r = nbest_check(h, "CTC beam search", W, N, n_hyp)) return r;
  if (int r = ctc_log_probs(h, encoded, B, Tp, nullptr, s)) return r;
  const int V = h->cfg.num_classes;
  return ctc_beam_launch(h, h->logits.p, enc_len, B, Tp, V, W, ids, frames, counts, score, logp, s, nbest, N, n_hyp);
}

int gam_ctc_beam(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, int W, int32_t* ids, int32_t* frames,
                 int32_t* counts, float* score, float* logp, void* stream) {
  return ctc_beam_run(h, encoded, enc_len, B, Tp, W, ids, frames, counts, score, logp, stream, false, 0, nullptr);
}

int gam_ctc_beam_nbest(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, int W, int N, int32_t* ids,
                       int32_t* frames, int32_t* counts, float* score, float* logp, int32_t* n_hyp, void* stream) {
  return ctc_beam_run(h, encoded, enc_len, B, Tp, W, ids, frames, counts, score, logp, stream, true, N, n_hyp);
}

int gam_op_ctc_beam_nbest(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, int W, int N,
                          int32_t* ids, int32_t* frames, int32_t* counts, float* score, float* logp, int32_t* n_hyp, void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  return ctc_beam_launch(h, log_probs, enc_len, B, Tp, V, W, ids, frames, counts, score, logp, s, true, N, n_hyp);
}

int gam_op_ctc_beam(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, int W, int32_t* ids,
                    int32_t* frames, int32_t* counts, float* score, float* logp, void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  return ctc_beam_launch(h, log_probs, enc_len, B, Tp, V, W, ids, frames, counts, score, logp, s);
}

// ---- the same search for one stream fed in pieces (gam_beam_stream.h gam_ctc_beam_stream_kernel).  Decode class as above; the state
// record and the node pool are the caller's.
int64_t gam_ctc_beam_stream_bytes(gam_handle* h, int W, int64_t max_frames) {
  if (!h) return -1;
  if (W < 1 || W > GAM_BEAM_MAX_W) return fail(h, -1, "CTC beam stream: beam width W=%d outside [1, %d]", W, GAM_BEAM_MAX_W);
  if (max_frames < 0 || max_frames * W >= 2147483648ll)
    return fail(h, -1, "CTC beam stream: max_frames=%lld x W=%d outside [0, 2^31)", (long long)max_frames, W);
  return (int64_t)GAM_BEAM_STREAM_HDR_BYTES + max_frames * W * (int64_t)sizeof(int4);
}

int gam_op_ctc_beam_stream(gam_handle* h, const float* log_probs, int64_t n, int V, int64_t t_base, int flags, int W, void* state,
                           int64_t state_bytes, int32_t* ids, int32_t* frames, int32_t* count, double* score, double* logp,
                           int32_t* status, void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  if (n < 0 || t_base < 0 || V < 2 || V > GAM_BEAM_MAX_V || n >= 2147483648ll || t_base >= 2147483648ll || t_base + n >= 2147483648ll)
    return fail(h, -1, "CTC beam stream: bad shape n=%lld V=%d t_base=%lld (t_base + n must stay below 2^31)", (long long)n, V,
                (long long)t_base);
  if (flags & ~(GAM_BEAM_F_BEGIN | GAM_BEAM_F_END)) return fail(h, -1, "CTC beam stream: unknown flags 0x%x", flags);
  if (int r = beam_check(h, "CTC beam stream", W, V, (n > 0 && !log_probs) || !state || !ids || !frames || !count || !score || !logp || !status,
                         "CTC beam stream: the LM's token classes are for V=%d, the log-probs have V=%d"))
    return r;
  if (state_bytes < (int64_t)GAM_BEAM_STREAM_HDR_BYTES)
    return fail(h, -1, "CTC beam stream: state_bytes=%lld below the record's %zu (gam_ctc_beam_stream_bytes)", (long long)state_bytes,
                (size_t)GAM_BEAM_STREAM_HDR_BYTES);
  // the frames the caller's pool holds at this W: the kernel refuses rows beyond them (and a state begun with more)
  const int64_t max_frames = std::min<int64_t>((state_bytes - (int64_t)GAM_BEAM_STREAM_HDR_BYTES) / ((int64_t)W * (int64_t)sizeof(int4)),
                                               2147483647ll / W);
  const int K = std::min(W, V - 1);
  const bool lm = h->lm_ng.p != nullptr;
  const bool hw_lds = h->hw_trie.p && (size_t)h->hw_words * 4 <= GAM_BEAM_HW_LDS_MAX;
  const size_t sm = gam_beam_lds_bytes(W, K, V, hw_lds ? h->hw_words : 0, lm);
  if (sm > 160 * 1024) return fail(h, -1, "CTC beam stream: %zu bytes of LDS exceed the limit %d", sm, 160 * 1024);
  GamBeamStreamArgs a;
  a.lp = log_probs; a.n = (int)n; a.t_base = (int)t_base; a.max_frames = (int)max_frames; a.flags = flags;
  a.V = V; a.W = W; a.K = K; a.hw_gen = h->hw_gen; a.lm_gen = h->lm_gen;
  a.hw = hw_args(h, hw_lds);
  a.lm = lm_args(h);
  a.state = state; a.ids = ids; a.frames = frames; a.count = count; a.score = score; a.logp = logp; a.status = status;
  static std::atomic<unsigned long long> lds_set[2];
  static const void* const kern[2] = {(const void*)gam_ctc_beam_stream_kernel<false>, (const void*)gam_ctc_beam_stream_kernel<true>};
  ProfScope ps(h, s, GAM_PF_DECODE, (double)n * W * (K + 1) * 4.0);
  return beam_launch(h, kern[lm ? 1 : 0], lds_set[lm ? 1 : 0], sm > 64 * 1024 ? 160 * 1024 : sm, 1, GAM_BEAM_NT, sm, s, &a);
}

int gam_set_hotwords(gam_handle* h, const int32_t* tokens, const int32_t* offsets, int n_phrases, float boost) {
  if (!h) return -1;
  if (n_phrases < 0 || n_phrases > GAM_BEAM_MAX_PHRASES)
    return fail(h, -1, "hotwords: %d phrases outside [0, %d]", n_phrases, GAM_BEAM_MAX_PHRASES);
  if (n_phrases > 0 && (!tokens || !offsets)) return fail(h, -1, "hotwords: NULL buffer");
  if (!std::isfinite(boost)) return fail(h, -1, "hotwords: boost is not finite");
  // the trie on the host: children per node (token -> child), phrase ends
  std::vector<std::map<int, int>> kids(1);
  std::vector<char> end(1, 0);
  int max_tok = -1;
  if (n_phrases > 0) {
    if (offsets[0] != 0) return fail(h, -1, "hotwords: offsets[0] = %d, expected 0", offsets[0]);
    const int hi = h->cfg.head_type == GAM_HEAD_CTC && h->cfg.num_classes >= 2 ? h->cfg.num_classes - 2 : GAM_BEAM_MAX_V - 2;
    for (int i = 0; i < n_phrases; ++i) {
      const int a = offsets[i], e = offsets[i + 1];
      if (e <= a) return fail(h, -1, "hotwords: phrase %d is empty or its offsets decrease", i);
      if (e > GAM_BEAM_MAX_HW_TOKENS) return fail(h, -1, "hotwords: more than %d tokens in all", GAM_BEAM_MAX_HW_TOKENS);
      int n = 0;
      for (int k = a; k < e; ++k) {
        const int c = tokens[k];
        if (c < 0 || c > hi) return fail(h, -1, "hotwords: token id %d of phrase %d outside [0, %d]", c, i, hi);
        max_tok = std::max(max_tok, c);
        auto it = kids[n].find(c);
        if (it == kids[n].end()) {
          kids.emplace_back();
          end.push_back(0);
          it = kids[n].emplace(c, (int)kids.size() - 1).first;
        }
        n = it->second;
      }
      end[n] = 1;
    }
  }
  // CSR: offsets [nodes + 1], then each node's edges in token order (token | end << 11 | child << 12)
  const int nn = (int)kids.size();
  std::vector<int> flat((size_t)nn + 1);
  int ne = 0;
  for (int n = 0; n < nn; ++n) {
    flat[n] = ne;
    ne += (int)kids[n].size();
  }
  flat[nn] = ne;
  for (int n = 0; n < nn; ++n)
    for (const auto& kv : kids[n]) flat.push_back(kv.first | (end[kv.second] << 11) | (kv.second << 12));
  HIPCHK(h, hipSetDevice(h->device));
  // a decode-class kernel still in flight may read the current trie
  if (h->dec_evt != nullptr && h->dec_evt_set) HIPCHK(h, hipEventSynchronize(h->dec_evt));
  ++h->hw_gen;
  if (n_phrases == 0) {
    h->hw_nodes = h->hw_words = 0;
    h->hw_max_tok = -1;
    HIPCHK(h, h->hw_trie.release());
    return 0;
  }
  if (int r = ensure_table(h, h->hw_trie, flat.size())) return r;
  HIPCHK(h, hipMemcpy(h->hw_trie.p, flat.data(), flat.size() * sizeof(int), hipMemcpyHostToDevice));
  h->hw_nodes = nn;
  h->hw_words = (int)flat.size();
  h->hw_max_tok = max_tok;
  h->hw_boost = boost;
  return 0;
}

static void lm_clear(gam_handle* h) {
  h->lm_cls = DevBuf(); h->lm_wt = DevBuf(); h->lm_ng = DevBuf();   // (the tables they held are freed)
  h->lm_V = 0;
}

int gam_set_lm(gam_handle* h, const int32_t* token_class, int V, const void* word_table, int64_t word_slots, int word_probe,
               const void* ngram_table, int64_t ngram_slots, int ngram_probe, int order, int bos, int eos, int unk, float unk_logp,
               float weight, float word_bonus) {
  if (!h) return -1;
  if (ngram_slots != 0) {
    const int64_t max_slots = (int64_t)1 << 30;
    auto pow2 = [](int64_t n) { return n > 0 && (n & (n - 1)) == 0; };
    if (order < 1 || order > GAM_BEAM_LM_MAX_ORDER) return fail(h, -1, "LM: order %d outside [1, %d]", order, GAM_BEAM_LM_MAX_ORDER);
    if (V < 2 || V > GAM_BEAM_MAX_V) return fail(h, -1, "LM: token classes for V=%d outside [2, %d]", V, GAM_BEAM_MAX_V);
    if (!token_class || !word_table || !ngram_table) return fail(h, -1, "LM: NULL buffer");
    for (int v = 0; v < V; ++v)
      if (token_class[v] < 0 || token_class[v] > 2) return fail(h, -1, "LM: token class %d of token %d outside [0, 2]", token_class[v], v);
    if (!pow2(word_slots) || !pow2(ngram_slots) || word_slots > max_slots || ngram_slots > max_slots)
      return fail(h, -1, "LM: table slots %lld / %lld must be powers of two <= 2^30", (long long)word_slots, (long long)ngram_slots);
    if (word_probe < 1 || word_probe > word_slots || ngram_probe < 1 || ngram_probe > ngram_slots)
      return fail(h, -1, "LM: probe bounds %d / %d outside [1, slots]", word_probe, ngram_probe);
    if (bos < 0 || eos < 0 || unk < 0 || bos >= (1 << 30) || eos >= (1 << 30) || unk >= (1 << 30))
      return fail(h, -1, "LM: word ids bos=%d eos=%d unk=%d outside [0, 2^30)", bos, eos, unk);
    if (!std::isfinite(unk_logp) || !std::isfinite(weight) || !std::isfinite(word_bonus))
      return fail(h, -1, "LM: unk_logp, weight and word bonus must be finite");
  }
  HIPCHK(h, hipSetDevice(h->device));
  // a decode-class kernel still in flight may read the current tables
  if (h->dec_evt != nullptr && h->dec_evt_set) HIPCHK(h, hipEventSynchronize(h->dec_evt));
  lm_clear(h);
  ++h->lm_gen;
  if (ngram_slots == 0) return 0;
  const size_t wb = (size_t)word_slots * 16, nbytes = (size_t)ngram_slots * 16;
  if (h->lm_cls.alloc((size_t)V) != hipSuccess || h->lm_wt.alloc(wb / 4) != hipSuccess || h->lm_ng.alloc(nbytes / 4) != hipSuccess) {
    lm_clear(h);
    return fail(h, -1, "LM: cannot allocate %zu bytes of device tables", (size_t)V * 4 + wb + nbytes);
  }
  if (hipMemcpy(h->lm_cls.p, token_class, (size_t)V * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->lm_wt.p, word_table, wb, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->lm_ng.p, ngram_table, nbytes, hipMemcpyHostToDevice) != hipSuccess) {
    lm_clear(h);
    return fail(h, -1, "LM: copying the tables to the device failed");
  }
  h->lm_V = V;
  h->lm_wslots = (int)word_slots; h->lm_wprobe = word_probe;
  h->lm_nslots = (int)ngram_slots; h->lm_nprobe = ngram_probe;
  h->lm_order = order; h->lm_bos = bos; h->lm_eos = eos; h->lm_unk = unk;
  h->lm_unk_logp = unk_logp; h->lm_alpha = weight; h->lm_beta = word_bonus;
  return 0;
}

// ---- RNN-T greedy decode: the argument block, the cluster plan, the kernel table, the two launches, the entry point
static GamRnntArgs rnnt_greedy_args(const gam_handle* h, const float* encp, const int32_t* enc_len, int B, int64_t Tp, int max_symbols,
                                    int32_t* ids, int32_t* frames, int32_t* counts, float* logits_dump, int32_t* dump_count, int dump_cap) {
  const gam_config& c = h->cfg;
  GamRnntArgs a;
  memset(&a, 0, sizeof a);
  rnnt_pred_weights(h, a);
  rnnt_joint_weights(h, a);
  a.encp = encp; a.enc_len = enc_len; a.ids = ids; a.frames = frames; a.counts = counts;
  a.dump = logits_dump; a.dump_count = dump_count; a.dump_cap = logits_dump ? dump_cap : 0;
  a.B = B; a.Tp = (int)Tp; a.V = c.num_classes; a.H = c.pred_hidden; a.JH = c.joint_hidden; a.L = c.pred_rnn_layers;
  a.max_symbols = max_symbols; a.cap = (int)Tp * max_symbols;
  return a;
}

// What the cluster decode (gam_decode_cluster.h) does with a shape: C workgroups per utterance in 8 utterance columns (one per XCD; the C
// members of a cluster share an XCD), grid <= one workgroup per CU.  C = 0 (and nothing else set): the one-workgroup kernel decodes it.
struct RnntClusterPlan {
  int C;                    // workgroups per utterance
  int need, nr;             // gate-row slots a thread needs (4 * ceil(H / C) rows over 256 threads), and the kernel's NR that holds them
  bool resident;            // W_hh rows register-resident (gam_decode_cluster.h RESQ)
  bool h320;                // H = JH = 320 at compile time (the published heads)
  int kern;                 // index into rnnt_cluster_kern
  int wout_slice_in_lds, wpred_slice_in_lds;
  size_t lds;               // dynamic LDS bytes of a workgroup
  size_t xg;                // exchange granules of the whole batch
  unsigned grid;            // workgroups
};

// Plain values in, no HIP call.  ncu: the device's CUs; cluster: gam_handle::rnnt_cluster (-1 auto); exclusive: GAM_RNNT_EXCLUSIVE.
static RnntClusterPlan rnnt_cluster_plan(int ncu, int cluster, int exclusive, int B, int H, int JH, int V, int L) {
  RnntClusterPlan p = {};
  const int nu8 = gam_cdiv(B, 8);
  // every member of every cluster must be resident at once (they spin on each other): at most one workgroup per CU
  // of THIS device, with a few CUs to spare; a partition with fewer CUs gets smaller clusters or the one-workgroup kernel
  int C = std::min(8, (ncu - 16) / (8 * nu8));
  if (cluster >= 0) C = std::min(cluster, C);
  if (C < 1 || JH % 16 != 0 || H % 4 != 0 || L != 1) return p;   // (JH % 16: MFMA k-steps and the LDS-DMA window; L > 1: one-workgroup kernel)
  const int need = gam_cdiv(4 * gam_cdiv(H, C), 256);
  if (need > 8) return p;
  static const int ladder[5] = {1, 2, 3, 5, 8};
  int col = 0;
  while (ladder[col] < need) ++col;
  const int nr = ladder[col];
  const int nV = gam_cdiv(gam_cdiv(V, C), 16) * 16;
  const int wout = (size_t)nV * (JH + 4) * 4 + gam_rnnt_cluster_smem(H, JH, V, C, nr, 0) <= 96 * 1024 ? 1 : 0;
  const int wpred = gam_rnnt_cluster_smem(H, JH, V, C, nr, wout, 1) <= 150 * 1024 ? 1 : 0;
  size_t lds = gam_rnnt_cluster_smem(H, JH, V, C, nr, wout, wpred);
  // GAM_RNNT_EXCLUSIVE=1: a decode workgroup asks for the CU's whole LDS (160 KB), so no other workgroup that uses LDS -- of this launch or
  // of ANOTHER stream's kernel -- is placed beside it.  r05 shipped this as the protection against a perturbation of co-resident decode
  // workgroups whose mechanism was unknown; r06 found it (hipcc had packed the gate rows' FMA chains into v_pk_fma_f32 op_sel:[0,1,0],
  // whose low result is wrong in lanes 48..63 beside another wave's MFMAs: gigaam_amd/build.py) and removed the instruction, so the
  // default is the kernel's own LDS size again; the switch stays as an A/B (profiles/r06_exclusive_ab.txt: no time difference).
  if (exclusive && lds <= 160 * 1024) lds = 160 * 1024;
  if (lds > 160 * 1024) return p;
  p.C = C; p.need = need; p.nr = nr;
  p.h320 = H == 320 && JH == 320;
  p.resident = p.h320 && nr == 1;
  p.kern = p.h320 && col < 4 ? col : 4 + col;
  p.wout_slice_in_lds = wout; p.wpred_slice_in_lds = wpred; p.lds = lds;
  p.xg = gam_rnnt_cluster_xgranules(H, JH, C) * (size_t)B;
  p.grid = (unsigned)(8 * nu8 * C);
  return p;
}

// One workgroup per utterance (gam_decode.h): the whole decode when the cluster kernel does not take the shape
// (GAM_RNNT_CLUSTER=0, a refused cluster launch), and -- with only_failed -- the REPAIR pass behind every cluster
// launch: a workgroup of it returns at once unless the cluster kernel left its utterance at counts[b] = -1 (a hand-off
// timed out because a member was not resident: GPU shared with another process / stream, CU-masked partition).  The
// caller therefore always gets the reference's ids back, without a host round trip and without an exception.
static int rnnt_single_launch(gam_handle* h, hipStream_t s, const GamRnntArgs& a, int only_failed) {
  GamRnntArgs f = a;
  f.only_failed = only_failed;
  f.wout_in_lds = gam_rnnt_smem(f.H, f.JH, f.V, 1, f.L) <= 96 * 1024 ? 1 : 0;
  size_t sm = gam_rnnt_smem(f.H, f.JH, f.V, f.wout_in_lds, f.L);
  if (h->rnnt_exclusive && f.B <= h->ncu && sm <= 160 * 1024) sm = 160 * 1024;   // (owns its CU like a cluster member: rnnt_cluster_plan)
  static std::atomic<unsigned long long> attr5{0}, attr8{0};
  HIPCHK(h, gam_set_max_lds(reinterpret_cast<const void*>(gam_rnnt_greedy_kernel<5>), 160 * 1024, attr5));
  HIPCHK(h, gam_set_max_lds(reinterpret_cast<const void*>(gam_rnnt_greedy_kernel<8>), 160 * 1024, attr8));
  if (sm > 160 * 1024) return fail(h, -1, "RNN-T head too large for the greedy kernel's LDS window");
  if (4 * f.H <= 256 * 5) hipLaunchKernelGGL(gam_rnnt_greedy_kernel<5>, dim3(f.B), dim3(256), sm, s, f);
  else hipLaunchKernelGGL(gam_rnnt_greedy_kernel<8>, dim3(f.B), dim3(256), sm, s, f);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// The cluster kernel's instantiations, each with the word that raises its LDS limit once per device.  [0..3]: H = JH = 320 at compile
// time, NR = 1 (resident), 2, 3, 5 (C = 1 there needs 5 slots: no NR = 8); [4..8]: the sizes as arguments, NR = 1, 2, 3, 5, 8.
static const void* const rnnt_cluster_kern[9] = {
    (const void*)gam_rnnt_cluster_kernel<1, 80>,     (const void*)gam_rnnt_cluster_kernel<2, 0, 320>, (const void*)gam_rnnt_cluster_kernel<3, 0, 320>,
    (const void*)gam_rnnt_cluster_kernel<5, 0, 320>, (const void*)gam_rnnt_cluster_kernel<1>,         (const void*)gam_rnnt_cluster_kernel<2>,
    (const void*)gam_rnnt_cluster_kernel<3>,         (const void*)gam_rnnt_cluster_kernel<5>,         (const void*)gam_rnnt_cluster_kernel<8>};
static std::atomic<unsigned long long> rnnt_cluster_kern_once[9];

// diagnosis build (-DGAM_RC_TIMING=1), GAM_RNNT_TIMING=1: the per-phase totals the kernel left behind the status word (utterance 0, member 0)
static int rnnt_timing_report(gam_handle* h, hipStream_t s, const int* status, const RnntClusterPlan& p) {
  if (!GAM_RC_TIMING || !getenv("GAM_RNNT_TIMING")) return 0;
  int st[16];
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipMemcpy(st, status, sizeof st, hipMemcpyDeviceToHost));
  fprintf(stderr, "[gam] rnnt cluster C=%d%s utt0: rounds %d; us: gates %.0f xH %.0f pred %.0f xP %.0f z %.0f joint %.0f xA %.0f comb %.0f ctrl %.0f\n", p.C,
          p.resident ? " (resident)" : "", st[T_ROUNDS], st[T_GATES] / 100.0, st[T_XH] / 100.0, st[T_PRED] / 100.0, st[T_XP] / 100.0, st[T_Z] / 100.0,
          st[T_JOINT] / 100.0, st[T_XA] / 100.0, st[T_COMB] / 100.0, st[T_CTRL] / 100.0);
  return 0;
}

// The cluster kernel over a planned shape (p.C >= 1).  *refused: the runtime did not take the launch and nothing was enqueued behind the
// memset; the caller decodes with rnnt_single_launch.
static int rnnt_cluster_launch(gam_handle* h, hipStream_t s, const GamRnntArgs& a, const RnntClusterPlan& p, bool* refused) {
  GamRnntClusterArgs ca;
  memset(&ca, 0, sizeof ca);
  ca.a = a; ca.whh_q = h->lstm_whh_q; ca.wpred_q = h->jn_pred_q; ca.C = p.C;
  ca.force_dead = h->rnnt_force_timeout;
  ca.wout_slice_in_lds = p.wout_slice_in_lds; ca.wpred_slice_in_lds = p.wpred_slice_in_lds;
  if (int r = ensure(h, h->rnnt_x, p.xg * 2 + 64)) return r;   // (floats: 2 per granule) + status word
  HIPCHK(h, hipMemsetAsync(h->rnnt_x.p, 0, (p.xg * 2 + 64) * sizeof(float), s));
  ca.xbuf = reinterpret_cast<unsigned long long*>(h->rnnt_x.p);
  ca.status = reinterpret_cast<int*>(h->rnnt_x.p + p.xg * 2);
  // Cooperative launch: the runtime REFUSES a grid that cannot be co-resident on this device (occupancy x CUs)
  // instead of letting resident members spin on absent ones; what it cannot see (CUs held by another queue) is
  // what the bounded spins + the repair pass are for.
  const bool coop = h->rnnt_coop != 0;
  const void* kern = rnnt_cluster_kern[p.kern];
  HIPCHK(h, gam_set_max_lds(kern, 160 * 1024, rnnt_cluster_kern_once[p.kern]));
  void* kargs[] = {&ca};
  const hipError_t le = coop ? hipLaunchCooperativeKernel(kern, dim3(p.grid), dim3(256), kargs, (unsigned)p.lds, s)
                             : hipLaunchKernel(kern, dim3(p.grid), dim3(256), kargs, p.lds, s);
  *refused = le != hipSuccess;
  if (*refused) {
    (void)hipGetLastError();
    static std::atomic<int> warned{0};
    if (!warned.exchange(1))
      fprintf(stderr, "[gam] RNN-T cluster decode: %s launch of %u workgroups refused (%s); decoding with one workgroup per utterance\n",
              coop ? "cooperative" : "plain", p.grid, hipGetErrorString(le));
    return 0;
  }
  return rnnt_timing_report(h, s, ca.status, p);
}

// The decode over a filled argument block: the cluster plan, the cluster launch with its repair pass, or the one-workgroup kernel.
static int rnnt_greedy_run(gam_handle* h, hipStream_t s, const GamRnntArgs& a) {
  const RnntClusterPlan p = rnnt_cluster_plan(h->ncu, h->rnnt_cluster, h->rnnt_exclusive, a.B, a.H, a.JH, a.V, a.L);
  ProfScope ps(h, s, GAM_PF_DECODE, 0.0);
  h->last_rnnt_c = p.C; h->last_rnnt_kern = p.C ? p.kern : -1; h->last_rnnt_refused = 0;   // (gam_rnnt_last_decode)
  if (p.C == 0) return rnnt_single_launch(h, s, a, 0);
  bool refused = false;
  if (int r = rnnt_cluster_launch(h, s, a, p, &refused)) return r;
  h->last_rnnt_refused = refused ? 1 : 0;
  if (refused) return rnnt_single_launch(h, s, a, 0);
  if (h->rnnt_no_repair) return 0;   // GAM_RNNT_NO_REPAIR=1 (test hook, read at gam_create): leave a failed cluster's counts at -1 (HipEngine.collect then raises)
  return rnnt_single_launch(h, s, a, 1);   // repair pass: no-op workgroups unless a cluster gave up
}

int gam_rnnt_greedy(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, int max_symbols,
                    int32_t* ids, int32_t* frames, int32_t* counts, float* logits_dump, int32_t* dump_count, int dump_cap,
                    void* stream) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "RNN-T head")) return r;
  if (B <= 0 || Tp <= 0 || max_symbols <= 0) return fail(h, -1, "bad arguments");
  GAM_DECODE_ENTRY(h, stream);
  if (int r = rnnt_encp(h, encoded, B, Tp, s)) return r;
  return rnnt_greedy_run(h, s, rnnt_greedy_args(h, h->encp.p, enc_len, B, Tp, max_symbols, ids, frames, counts, logits_dump, dump_count, dump_cap));
}

// gam_rnnt_greedy from a caller-supplied encoder projection: the same plan, no logits dump.
int gam_op_rnnt_greedy(gam_handle* h, const float* encp, const int32_t* enc_len, int B, int64_t Tp, int max_symbols, int32_t* ids,
                       int32_t* frames, int32_t* counts, void* stream) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "RNN-T head")) return r;
  if (B <= 0 || Tp <= 0 || max_symbols <= 0 || Tp * max_symbols >= 2147483648ll) return fail(h, -1, "bad arguments");
  if (!encp || !enc_len || !ids || !frames || !counts) return fail(h, -1, "RNN-T greedy decode: NULL buffer");
  GAM_DECODE_ENTRY(h, stream);
  return rnnt_greedy_run(h, s, rnnt_greedy_args(h, encp, enc_len, B, Tp, max_symbols, ids, frames, counts, nullptr, nullptr, 0));
}

// The encoder projection GEMM of gam_rnnt_greedy into the caller's buffer.
int gam_rnnt_encp(gam_handle* h, const float* encoded, int B, int64_t Tp, float* encp_out, void* stream) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "RNN-T head")) return r;
  if (B <= 0 || Tp <= 0) return fail(h, -1, "bad shape B=%d T'=%lld", B, (long long)Tp);
  if (!encoded || !encp_out) return fail(h, -1, "RNN-T encoder projection: NULL buffer");
  GAM_DECODE_ENTRY(h, stream);
  return rnnt_encp(h, encoded, B, Tp, s, encp_out);
}

// ---- the greedy decode of one stream fed in pieces (gam_rnnt_stream.h gam_rnnt_greedy_stream_kernel).  Decode class as above; the
// state record and the result arrays are the caller's.
int64_t gam_rnnt_greedy_stream_bytes(gam_handle* h) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "RNN-T head")) return r;
  return (int64_t)gam_rnnt_stream_bytes(h->cfg.pred_hidden, h->cfg.pred_rnn_layers);
}

int gam_op_rnnt_greedy_stream(gam_handle* h, const float* encp, int64_t n, int64_t t_base, int flags, int max_symbols, void* state,
                              int64_t state_bytes, int32_t* ids, int32_t* frames, int64_t cap, int32_t* count, int32_t* status,
                              void* stream) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "RNN-T head")) return r;
  if (n < 0 || t_base < 0 || n >= 2147483648ll || t_base >= 2147483648ll || t_base + n >= 2147483648ll)
    return fail(h, -1, "RNN-T greedy stream: bad shape n=%lld t_base=%lld (t_base + n must stay below 2^31)", (long long)n, (long long)t_base);
  if (max_symbols < 1 || cap < 0) return fail(h, -1, "RNN-T greedy stream: max_symbols=%d below 1 or cap=%lld below 0", max_symbols, (long long)cap);
  if (flags & ~(GAM_RNNT_F_BEGIN | GAM_RNNT_F_END)) return fail(h, -1, "RNN-T greedy stream: unknown flags 0x%x", flags);
  if ((n > 0 && !encp) || !state || !ids || !frames || !count || !status) return fail(h, -1, "RNN-T greedy stream: NULL buffer");
  const int64_t need_bytes = (int64_t)gam_rnnt_stream_bytes(h->cfg.pred_hidden, h->cfg.pred_rnn_layers);
  if (state_bytes < need_bytes)
    return fail(h, -1, "RNN-T greedy stream: state_bytes=%lld below the record's %lld (gam_rnnt_greedy_stream_bytes)", (long long)state_bytes,
                (long long)need_bytes);
  GamRnntStreamArgs g;
  memset(&g, 0, sizeof g);
  rnnt_pred_weights(h, g.a);
  rnnt_joint_weights(h, g.a);
  const gam_config& c = h->cfg;
  GamRnntArgs& a = g.a;
  a.encp = encp; a.ids = ids; a.frames = frames;
  a.B = 1; a.Tp = (int)n; a.V = c.num_classes; a.H = c.pred_hidden; a.JH = c.joint_hidden; a.L = c.pred_rnn_layers;
  a.max_symbols = max_symbols; a.cap = (int)std::min<int64_t>(cap, 2147483647ll);
  a.wout_in_lds = gam_rnnt_smem(a.H, a.JH, a.V, 1, a.L) <= 96 * 1024 ? 1 : 0;      // (the batch kernel's rule: rnnt_single_launch)
  const size_t sm = gam_rnnt_smem(a.H, a.JH, a.V, a.wout_in_lds, a.L);
  if (sm > 160 * 1024) return fail(h, -1, "RNN-T head too large for the greedy kernel's LDS window");
  g.n = (int)n; g.t_base = (int)t_base; g.flags = flags; g.state = state; g.count = count; g.status = status;
  GAM_DECODE_ENTRY(h, stream);
  static std::atomic<unsigned long long> attr5{0}, attr8{0};
  HIPCHK(h, gam_set_max_lds(reinterpret_cast<const void*>(gam_rnnt_greedy_stream_kernel<5>), 160 * 1024, attr5));
  HIPCHK(h, gam_set_max_lds(reinterpret_cast<const void*>(gam_rnnt_greedy_stream_kernel<8>), 160 * 1024, attr8));
  ProfScope ps(h, s, GAM_PF_DECODE, 0.0);
  if (4 * a.H <= 256 * 5) hipLaunchKernelGGL(gam_rnnt_greedy_stream_kernel<5>, dim3(1), dim3(256), sm, s, g);
  else hipLaunchKernelGGL(gam_rnnt_greedy_stream_kernel<8>, dim3(1), dim3(256), sm, s, g);
  HIPCHK(h, hipGetLastError());
  return 0;
}
// RNN-T beam search over the encoder projection encp [B, Tp, JH] (gam_rnnt_beam.h): one workgroup per utterance; with the handle's LM
// (gam_set_lm) gam_rnnt_beam_kernel<true>.  Decode class (the caller holds a DecodeScope): the state slots, logit rows and prefix-trie
// nodes are the handle's.  nbest: the <.., true> kernels, ids / frames [B, N, cap] and counts / score / logp [B, N]; else N and n_hyp
// are not read.
static int rnnt_beam_launch(gam_handle* h, const float* encp, const int32_t* enc_len, int B, int64_t Tp, int W, int max_symbols,
                            int32_t* ids, int32_t* frames, int32_t* counts, float* score, float* logp, hipStream_t s, bool nbest = false,
                            int N = 0, int32_t* n_hyp = nullptr) {
  const gam_config& c = h->cfg;
  const int V = c.num_classes, H = c.pred_hidden, JH = c.joint_hidden, L = c.pred_rnn_layers;
  if (B <= 0 || Tp <= 0) return fail(h, -1, "RNN-T beam search: bad shape B=%d T'=%lld", B, (long long)Tp);
  if (Tp > GAM_RB_MAX_T) return fail(h, -1, "RNN-T beam search: T'=%lld frames exceed the limit %d", (long long)Tp, GAM_RB_MAX_T);
  if (max_symbols < 1 || max_symbols > GAM_RB_MAX_S)
    return fail(h, -1, "RNN-T beam search: max_symbols S=%d outside [1, %d]", max_symbols, GAM_RB_MAX_S);
  if (V < 2 || V > GAM_BEAM_MAX_V) return fail(h, -1, "RNN-T beam search: V=%d outside [2, %d]", V, GAM_BEAM_MAX_V);
  if (H > GAM_RB_MAX_H || JH > GAM_RB_MAX_H || H % 16 != 0 || JH % 16 != 0)
    return fail(h, -1, "RNN-T beam search: H=%d / JH=%d must be multiples of 16 up to %d", H, JH, GAM_RB_MAX_H);
  if (int r = beam_check(h, "RNN-T beam search", W, V, !encp || !enc_len || !ids || !frames || !counts || !score || !logp,
                         "RNN-T beam search: the LM's token classes are for V=%d, the model has V=%d"))
    return r;
  if (nbest)
    if (int r = nbest_check(h, "RNN-T beam search", W, N, n_hyp)) return r;
  const bool lm = h->lm_ng.p != nullptr;
  const int K = std::min(W, V - 1);
  const size_t base = gam_rb_lds_bytes(W, K, max_symbols, H, JH, L, 0, lm ? V : 0);
  if (base > 160 * 1024)
    return fail(h, -1, "RNN-T beam search: W=%d, S=%d, H=%d, L=%d%s need %zu bytes of LDS (> 160 KiB)", W, max_symbols, H, L,
                lm ? " with the LM" : "", base);
  const bool hw_lds = h->hw_trie.p && (size_t)h->hw_words * 4 <= GAM_BEAM_HW_LDS_MAX && base + (size_t)h->hw_words * 4 <= 160 * 1024;
  const size_t sm = gam_rb_lds_bytes(W, K, max_symbols, H, JH, L, hw_lds ? h->hw_words : 0, lm ? V : 0);
  const size_t per = (gam_rb_ws_floats(W, max_symbols, V, H, JH, L) + 63) & ~(size_t)63;
  if (int r = ensure(h, h->rb_ws, per * B + 64)) return r;
  if (int r = ensure(h, h->rb_nodes, (size_t)B * Tp * max_symbols * W * 2 + 64)) return r;
  GamRnntBeamArgs a;
  memset(&a, 0, sizeof a);
  rnnt_pred_weights(h, a);
  rnnt_joint_weights(h, a);
  a.encp = encp; a.enc_len = enc_len;
  a.Tp = (int)Tp; a.V = V; a.H = H; a.JH = JH; a.L = L; a.W = W; a.K = K; a.S = max_symbols;
  a.hw = hw_args(h, hw_lds);
  a.lm = lm_args(h);
  a.ws = h->rb_ws.p; a.ws_stride = per;
  a.nodes = reinterpret_cast<int2*>(h->rb_nodes.p);
  a.ids = ids; a.frames = frames; a.cap = (int)Tp * max_symbols; a.counts = counts; a.score = score; a.logp = logp;
  a.nb.n_hyp = nbest ? n_hyp : nullptr; a.nb.n = nbest ? N : 0;
  static std::atomic<unsigned long long> lds_set[4];
  static const void* const kern[4] = {(const void*)gam_rnnt_beam_kernel<false, false>, (const void*)gam_rnnt_beam_kernel<true, false>,
                                      (const void*)gam_rnnt_beam_kernel<false, true>, (const void*)gam_rnnt_beam_kernel<true, true>};
  const int ki = (lm ? 1 : 0) + (nbest ? 2 : 0);
  ProfScope ps(h, s, GAM_PF_DECODE, (double)B * Tp * ((double)V * JH + 4.0 * H * H) * 4.0);
  return beam_launch(h, kern[ki], lds_set[ki], 160 * 1024, B, GAM_RB_NT, sm, s, &a);
}

// gam_rnnt_beam / gam_rnnt_beam_nbest: the encoder projection GEMM, the beam kernel.
static int rnnt_beam_run(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, int W, int max_symbols,
                         int32_t* ids, int32_t* frames, int32_t* counts, float* score, float* logp, void* stream, bool nbest, int N,
                         int32_t* n_hyp) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "RNN-T head")) return r;
  GAM_DECODE_ENTRY(h, stream);
  if (B <= 0 || Tp <= 0 || Tp > GAM_RB_MAX_T || W < 1 || W > GAM_BEAM_MAX_W || max_symbols < 1 || max_symbols > GAM_RB_MAX_S)
    return fail(h, -1, "RNN-T beam search: B=%d T'=%lld / W=%d / S=%d beyond the limits (%d / [1, %d] / [1, %d])", B, (long long)Tp, W,
                max_symbols, GAM_RB_MAX_T, GAM_BEAM_MAX_W, GAM_RB_MAX_S);
  if (nbest)
    if (int r = nbest_check(h, "RNN-T beam search", W, N, n_hyp)) return r;
  if (int r = rnnt_encp(h, encoded, B, Tp, s)) return r;
  return rnnt_beam_launch(h, h->encp.p, enc_len, B, Tp, W, max_symbols, ids, frames, counts, score, logp, s, nbest, N, n_hyp);
}

int gam_rnnt_beam(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, int W, int max_symbols, int32_t* ids,
                  int32_t* frames, int32_t* counts, float* score, float* logp, void* stream) {
  return rnnt_beam_run(h, encoded, enc_len, B, Tp, W, max_symbols, ids, frames, counts, score, logp, stream, false, 0, nullptr);
}

int gam_rnnt_beam_nbest(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, int W, int max_symbols, int N,
                        int32_t* ids, int32_t* frames, int32_t* counts, float* score, float* logp, int32_t* n_hyp, void* stream) {
  return rnnt_beam_run(h, encoded, enc_len, B, Tp, W, max_symbols, ids, frames, counts, score, logp, stream, true, N, n_hyp);
}

int gam_op_rnnt_beam_nbest(gam_handle* h, const float* encp, const int32_t* enc_len, int B, int64_t Tp, int W, int max_symbols, int N,
                           int32_t* ids, int32_t* frames, int32_t* counts, float* score, float* logp, int32_t* n_hyp, void* stream) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "RNN-T head")) return r;
  GAM_DECODE_ENTRY(h, stream);
  return rnnt_beam_launch(h, encp, enc_len, B, Tp, W, max_symbols, ids, frames, counts, score, logp, s, true, N, n_hyp);
}

int gam_op_rnnt_beam(gam_handle* h, const float* encp, const int32_t* enc_len, int B, int64_t Tp, int W, int max_symbols, int32_t* ids,
                     int32_t* frames, int32_t* counts, float* score, float* logp, void* stream) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "RNN-T head")) return r;
  GAM_DECODE_ENTRY(h, stream);
  return rnnt_beam_launch(h, encp, enc_len, B, Tp, W, max_symbols, ids, frames, counts, score, logp, s);
}

// ---- the same search for one stream fed in pieces (gam_rnnt_beam_stream.h gam_rnnt_beam_stream_kernel).  Decode class as above; the
// state record with its slot and node pools is the caller's, the logit rows are the handle's.
// The limits both stream entries share; K and the head's sizes for the caller.
static int rnnt_beam_stream_check(gam_handle* h, int W, int max_symbols) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "RNN-T head")) return r;
  const gam_config& c = h->cfg;
  const int V = c.num_classes, H = c.pred_hidden, JH = c.joint_hidden;
  if (W < 1 || W > GAM_BEAM_MAX_W) return fail(h, -1, "RNN-T beam stream: beam width W=%d outside [1, %d]", W, GAM_BEAM_MAX_W);
  if (max_symbols < 1 || max_symbols > GAM_RB_MAX_S)
    return fail(h, -1, "RNN-T beam stream: max_symbols S=%d outside [1, %d]", max_symbols, GAM_RB_MAX_S);
  if (V < 2 || V > GAM_BEAM_MAX_V) return fail(h, -1, "RNN-T beam stream: V=%d outside [2, %d]", V, GAM_BEAM_MAX_V);
  if (H > GAM_RB_MAX_H || JH > GAM_RB_MAX_H || H % 16 != 0 || JH % 16 != 0)
    return fail(h, -1, "RNN-T beam stream: H=%d / JH=%d must be multiples of 16 up to %d", H, JH, GAM_RB_MAX_H);
  return 0;
}

int64_t gam_rnnt_beam_stream_bytes(gam_handle* h, int W, int max_symbols, int64_t max_frames) {
  if (int r = rnnt_beam_stream_check(h, W, max_symbols)) return r;
  if (max_frames < 0 || max_frames * max_symbols * W >= 2147483648ll)
    return fail(h, -1, "RNN-T beam stream: max_frames=%lld x S=%d x W=%d outside [0, 2^31)", (long long)max_frames, max_symbols, W);
  const gam_config& c = h->cfg;
  return (int64_t)gam_rb_stream_fixed_bytes(W, max_symbols, c.pred_hidden, c.joint_hidden, c.pred_rnn_layers) +
         max_frames * max_symbols * W * (int64_t)sizeof(int4);
}

int gam_op_rnnt_beam_stream(gam_handle* h, const float* encp, int64_t n, int64_t t_base, int flags, int W, int max_symbols, void* state,
                            int64_t state_bytes, int32_t* ids, int32_t* frames, int64_t cap, int32_t* count, double* score, double* logp,
                            int32_t* status, void* stream) {
  if (int r = rnnt_beam_stream_check(h, W, max_symbols)) return r;
  GAM_DECODE_ENTRY(h, stream);
  const gam_config& c = h->cfg;
  const int V = c.num_classes, H = c.pred_hidden, JH = c.joint_hidden, L = c.pred_rnn_layers;
  if (n < 0 || t_base < 0 || n >= 2147483648ll || t_base >= 2147483648ll || t_base + n >= 2147483648ll)
    return fail(h, -1, "RNN-T beam stream: bad shape n=%lld t_base=%lld (t_base + n must stay below 2^31)", (long long)n, (long long)t_base);
  if (cap < 0) return fail(h, -1, "RNN-T beam stream: cap=%lld below 0", (long long)cap);
  if (flags & ~(GAM_RB_F_BEGIN | GAM_RB_F_END)) return fail(h, -1, "RNN-T beam stream: unknown flags 0x%x", flags);
  if (int r = beam_check(h, "RNN-T beam stream", W, V, (n > 0 && !encp) || !state || !ids || !frames || !count || !score || !logp || !status,
                         "RNN-T beam stream: the LM's token classes are for V=%d, the model has V=%d"))
    return r;
  if (reinterpret_cast<uintptr_t>(state) & 15)      // (the entries' word state and the nodes are int4)
    return fail(h, -1, "RNN-T beam stream: state %p is not 16-byte aligned", state);
  const int64_t fixed = (int64_t)gam_rb_stream_fixed_bytes(W, max_symbols, H, JH, L);
  if (state_bytes < fixed)
    return fail(h, -1, "RNN-T beam stream: state_bytes=%lld below the record's %lld (gam_rnnt_beam_stream_bytes)", (long long)state_bytes,
                (long long)fixed);
  // the frames the caller's node pool holds at this W and S: the kernel refuses rows beyond them (and a record begun with more)
  const int64_t per_frame = (int64_t)max_symbols * W;
  const int64_t max_frames = std::min<int64_t>((state_bytes - fixed) / (per_frame * (int64_t)sizeof(int4)), 2147483647ll / per_frame);
  const bool lm = h->lm_ng.p != nullptr;
  const int K = std::min(W, V - 1);
  const size_t base = gam_rb_lds_bytes(W, K, max_symbols, H, JH, L, 0, lm ? V : 0);
  if (base > 160 * 1024)
    return fail(h, -1, "RNN-T beam stream: W=%d, S=%d, H=%d, L=%d%s need %zu bytes of LDS (> 160 KiB)", W, max_symbols, H, L,
                lm ? " with the LM" : "", base);
  const bool hw_lds = h->hw_trie.p && (size_t)h->hw_words * 4 <= GAM_BEAM_HW_LDS_MAX && base + (size_t)h->hw_words * 4 <= 160 * 1024;
  const size_t sm = gam_rb_lds_bytes(W, K, max_symbols, H, JH, L, hw_lds ? h->hw_words : 0, lm ? V : 0);
  if (int r = ensure(h, h->rb_ws, gam_rb_stream_ws_floats(W, V) + 64)) return r;
  GamRnntBeamStreamArgs g;
  memset(&g, 0, sizeof g);
  GamRnntBeamArgs& a = g.a;
  rnnt_pred_weights(h, a);
  rnnt_joint_weights(h, a);
  a.encp = encp;
  a.Tp = (int)n; a.V = V; a.H = H; a.JH = JH; a.L = L; a.W = W; a.K = K; a.S = max_symbols;
  a.hw = hw_args(h, hw_lds);
  a.lm = lm_args(h);
  a.ws = h->rb_ws.p;
  a.ids = ids; a.frames = frames; a.cap = (int)std::min<int64_t>(cap, 2147483647ll); a.counts = count;
  g.x.n = (int)n; g.x.t_base = (int)t_base; g.x.max_frames = (int)max_frames; g.x.flags = flags;
  g.x.hw_gen = h->hw_gen; g.x.lm_gen = h->lm_gen;
  g.x.state = state; g.x.status = status; g.x.score = score; g.x.logp = logp;
  static std::atomic<unsigned long long> lds_set[2];
  static const void* const kern[2] = {(const void*)gam_rnnt_beam_stream_kernel<false>, (const void*)gam_rnnt_beam_stream_kernel<true>};
  ProfScope ps(h, s, GAM_PF_DECODE, (double)n * ((double)V * JH + 4.0 * H * H) * 4.0);
  return beam_launch(h, kern[lm ? 1 : 0], lds_set[lm ? 1 : 0], 160 * 1024, 1, GAM_RB_NT, sm, s, &g);
}

// ---- transducer forced alignment (gam_rnnt_align.h).  Decode class (the caller holds a DecodeScope): every buffer is the handle's.
// The lattice sweep over (lb, le) float2 [B, Tp, Umax + 1]: one workgroup per utterance.
static int rnnt_lattice_dp_launch(gam_handle* h, const float2* lat, const int32_t* enc_len, int B, int64_t Tp, int V, const int32_t* targets,
                                  const int32_t* target_len, int Umax, int32_t* tok_frame, float* score, float* loglik, int32_t* status,
                                  hipStream_t s) {
  const int u1 = Umax + 1;
  const int nt = std::min(GAM_RA_MAX_NT, std::max(64, (u1 + 63) / 64 * 64));
  const int spt = (u1 + nt - 1) / nt;
  const int nchunk = (u1 + 63) / 64;
  const bool bp_lds = gam_ra_dp_lds_bytes(true, (int)Tp, Umax, nchunk, spt, nt) <= GAM_RA_LDS_MAX;
  const size_t sm = gam_ra_dp_lds_bytes(bp_lds, (int)Tp, Umax, nchunk, spt, nt);
  GamRnntDpArgs a;
  a.lat = lat; a.enc_len = enc_len; a.targets = targets; a.target_len = target_len;
  a.Tp = (int)Tp; a.Umax = Umax; a.V = V; a.nchunk = nchunk; a.bp_glob = nullptr;
  a.tok_frame = tok_frame; a.score = score; a.loglik = loglik; a.status = status;
  if (!bp_lds) {
    if (int r = ensure(h, h->ra_bp, (size_t)B * (Tp + Umax) * nchunk * 2 + 64)) return r;
    a.bp_glob = reinterpret_cast<unsigned long long*>(h->ra_bp.p);
  }
  static std::atomic<unsigned long long> lds_set[4];
  const int which = (bp_lds ? 2 : 0) + (spt - 1);
  void (*const kerns[4])(GamRnntDpArgs) = {gam_rnnt_lattice_dp_kernel<false, 1>, gam_rnnt_lattice_dp_kernel<false, 2>,
                                           gam_rnnt_lattice_dp_kernel<true, 1>, gam_rnnt_lattice_dp_kernel<true, 2>};
  if (sm > 64 * 1024) HIPCHK(h, gam_set_max_lds((const void*)kerns[which], GAM_RA_LDS_MAX, lds_set[which]));
  ProfScope ps(h, s, GAM_PF_DECODE, (double)B * Tp * u1 * 8.0);
  hipLaunchKernelGGL(kerns[which], dim3(B), dim3(nt), sm, s, a);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// The predictor half of the joint for given label sequences: the teacher-forced predictor g = h->ra_g [B, Umax + 1, H] (gam_rnnt_align.h),
// then pp = W_pred g + b_pred = h->ra_pp [B, Umax + 1, JH].  The caller has checked H, JH and L against the kernel's limits.
static int rnnt_tf_pp(gam_handle* h, const int32_t* targets, const int32_t* target_len, int B, int Umax, hipStream_t s) {
  const gam_config& c = h->cfg;
  const int V = c.num_classes, H = c.pred_hidden, JH = c.joint_hidden, L = c.pred_rnn_layers, u1 = Umax + 1;
  if (int r = ensure(h, h->ra_g, (size_t)B * u1 * H + 64)) return r;
  if (int r = ensure(h, h->ra_pp, (size_t)B * u1 * JH + 64)) return r;
  {
    GamRnntTfArgs a;
    rnnt_pred_weights(h, a);
    a.targets = targets; a.target_len = target_len; a.g = h->ra_g.p; a.Umax = Umax; a.V = V; a.H = H; a.L = L;
    ProfScope ps(h, s, GAM_PF_DECODE, (double)B * u1 * L * 8.0 * H * H * 4.0);
    const size_t sm = gam_ra_tf_lds_bytes(H, L);
    if (4 * H <= 256 * 5) hipLaunchKernelGGL(gam_rnnt_tf_predict_kernel<5>, dim3(B), dim3(256), sm, s, a);
    else hipLaunchKernelGGL(gam_rnnt_tf_predict_kernel<8>, dim3(B), dim3(256), sm, s, a);
    HIPCHK(h, hipGetLastError());
  }
  GamGemmArgs gp = gemm_args(h->ra_g.p, H, h->jn_pred_w, h->jn_pred_b, h->ra_pp.p, JH, B * u1, JH, H);
  return gemm(h, s, gp, GAM_ACT_NONE, GAM_PF_DECODE);
}

static int rnnt_align_shape_check(gam_handle* h, int B, int64_t Tp, int Umax, int V, bool null_buf) {
  if (B <= 0 || Tp <= 0 || V < 2) return fail(h, -1, "RNN-T alignment: bad shape B=%d T'=%lld V=%d", B, (long long)Tp, V);
  if (Tp > GAM_RA_MAX_T) return fail(h, -1, "RNN-T alignment: T'=%lld frames exceed the limit %d", (long long)Tp, GAM_RA_MAX_T);
  if (Umax < 0 || Umax > GAM_RA_MAX_U) return fail(h, -1, "RNN-T alignment: Umax=%d tokens outside [0, %d]", Umax, GAM_RA_MAX_U);
  if (V > GAM_BEAM_MAX_V) return fail(h, -1, "RNN-T alignment: V=%d outside [2, %d]", V, GAM_BEAM_MAX_V);
  if (null_buf) return fail(h, -1, "RNN-T alignment: NULL buffer");
  return 0;
}

// The whole alignment from the encoder projection encp [B, Tp, JH]: predictor, its projection, then per slice of utterances the fused
// lattice kernel and the sweep.  lattice_out (may be NULL): a copy of the (lb, le) lattice, [B, Tp, Umax + 1] float2.
static int rnnt_align_launch(gam_handle* h, const float* encp, const int32_t* enc_len, int B, int64_t Tp, const int32_t* targets,
                             const int32_t* target_len, int Umax, int32_t* tok_frame, float* score, float* loglik, int32_t* status,
                             float* lattice_out, hipStream_t s) {
  const gam_config& c = h->cfg;
  const int V = c.num_classes, H = c.pred_hidden, JH = c.joint_hidden, L = c.pred_rnn_layers;
  if (int r = rnnt_align_shape_check(h, B, Tp, Umax, V,
                                     !encp || !enc_len || !target_len || !score || !loglik || !status || (Umax > 0 && (!targets || !tok_frame))))
    return r;
  if (H > GAM_RA_MAX_H || JH > GAM_RA_MAX_H || H % 16 != 0 || JH % 16 != 0 || L < 1 || L > 4)
    return fail(h, -1, "RNN-T alignment: H=%d / JH=%d must be multiples of 16 up to %d, 1..4 predictor layers (L=%d)", H, JH, GAM_RA_MAX_H, L);
  const int u1 = Umax + 1;
  const size_t per = (size_t)Tp * u1 * sizeof(float2);      // lattice bytes of one utterance
  if (per > h->ra_ws_limit)
    return fail(h, -1, "RNN-T alignment: the lattice of one utterance (T'=%lld x %d nodes) takes %zu bytes, the workspace limit is %zu bytes",
                (long long)Tp, u1, per, h->ra_ws_limit);
  const int nb = (int)std::min<size_t>((size_t)B, h->ra_ws_limit / per);
  if (int r = rnnt_tf_pp(h, targets, target_len, B, Umax, s)) return r;
  if (int r = ensure(h, h->ra_lat, (size_t)nb * Tp * u1 * 2 + 64)) return r;
  static std::atomic<unsigned long long> lds_set;
  const size_t sml = gam_ra_lat_lds_bytes(JH);
  if (sml > 64 * 1024) HIPCHK(h, gam_set_max_lds((const void*)gam_rnnt_lattice_kernel, GAM_RA_LDS_MAX, lds_set));
  for (int b0 = 0; b0 < B; b0 += nb) {
    const int n = std::min(nb, B - b0);
    GamRnntLatArgs a;
    a.encp = encp + (size_t)b0 * Tp * JH; a.predp = h->ra_pp.p + (size_t)b0 * u1 * JH; a.enc_len = enc_len + b0;
    a.targets = targets ? targets + (size_t)b0 * Umax : nullptr; a.target_len = target_len + b0; a.wout = h->jn_out_w; a.bout = h->jn_out_b;
    a.lat = reinterpret_cast<float2*>(h->ra_lat.p); a.Tp = (int)Tp; a.Umax = Umax; a.V = V; a.JH = JH;
    {
      ProfScope ps(h, s, GAM_PF_DECODE, (double)n * Tp * u1 * ((double)V * JH * 2.0));
      hipLaunchKernelGGL(gam_rnnt_lattice_kernel, dim3(gam_cdiv(Tp, GAM_RA_TF), gam_cdiv(u1, 16), n), dim3(256), sml, s, a);
      HIPCHK(h, hipGetLastError());
    }
    if (lattice_out)
      HIPCHK(h, hipMemcpyAsync(lattice_out + (size_t)b0 * Tp * u1 * 2, h->ra_lat.p, (size_t)n * per, hipMemcpyDeviceToDevice, s));
    if (int r = rnnt_lattice_dp_launch(h, a.lat, a.enc_len, n, Tp, V, a.targets, a.target_len, Umax,
                                       tok_frame ? tok_frame + (size_t)b0 * Umax : nullptr, score + b0, loglik + b0, status + b0, s))
      return r;
  }
  return 0;
}

int gam_rnnt_align(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, const int32_t* targets,
                   const int32_t* target_len, int Umax, int32_t* tok_frame, float* score, float* loglik, int32_t* status, void* stream) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "RNN-T head")) return r;
  GAM_DECODE_ENTRY(h, stream);
  if (int r = rnnt_align_shape_check(h, B, Tp, Umax, h->cfg.num_classes, !encoded)) return r;
  if (int r = rnnt_encp(h, encoded, B, Tp, s)) return r;
  return rnnt_align_launch(h, h->encp.p, enc_len, B, Tp, targets, target_len, Umax, tok_frame, score, loglik, status, nullptr, s);
}

int gam_op_rnnt_align(gam_handle* h, const float* encp, const int32_t* enc_len, int B, int64_t Tp, const int32_t* targets,
                      const int32_t* target_len, int Umax, int32_t* tok_frame, float* score, float* loglik, int32_t* status,
                      float* lattice_out, void* stream) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "RNN-T head")) return r;
  GAM_DECODE_ENTRY(h, stream);
  return rnnt_align_launch(h, encp, enc_len, B, Tp, targets, target_len, Umax, tok_frame, score, loglik, status, lattice_out, s);
}

int gam_op_rnnt_lattice_align(gam_handle* h, const float* lattice, const int32_t* enc_len, int B, int64_t Tp, int V, const int32_t* targets,
                              const int32_t* target_len, int Umax, int32_t* tok_frame, float* score, float* loglik, int32_t* status,
                              void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  if (int r = rnnt_align_shape_check(h, B, Tp, Umax, V,
                                     !lattice || !enc_len || !target_len || !score || !loglik || !status || (Umax > 0 && !tok_frame)))
    return r;
  return rnnt_lattice_dp_launch(h, reinterpret_cast<const float2*>(lattice), enc_len, B, Tp, V, targets, target_len, Umax, tok_frame, score,
                                loglik, status, s);
}

int gam_set_rnnt_align_workspace(gam_handle* h, int64_t bytes) {
  if (!h) return -1;
  if (bytes < 0) return fail(h, -1, "RNN-T alignment: workspace limit %lld bytes is negative", (long long)bytes);
  h->ra_ws_limit = bytes == 0 ? GAM_RA_WS_DEFAULT : (size_t)bytes;
  return 0;
}

// ---- token confidence of a finished decode (gam_confidence.h).  Decode class (the caller holds a DecodeScope): every buffer is the handle's.
static int conf_shape_check(gam_handle* h, const char* what, int B, int64_t Tp, int V, int cap, int cap_max, int measure, int agg, bool null_buf) {
  if (B <= 0 || Tp <= 0 || V < 2) return fail(h, -1, "%s confidence: bad shape B=%d T'=%lld V=%d", what, B, (long long)Tp, V);
  if (Tp > GAM_CF_MAX_T) return fail(h, -1, "%s confidence: T'=%lld frames exceed the limit %d", what, (long long)Tp, GAM_CF_MAX_T);
  if (V > GAM_CF_MAX_V) return fail(h, -1, "%s confidence: V=%d outside [2, %d]", what, V, GAM_CF_MAX_V);
  if (cap < 0 || cap > cap_max) return fail(h, -1, "%s confidence: cap=%d tokens outside [0, %d]", what, cap, cap_max);
  if (measure != GAM_CF_PROB && measure != GAM_CF_ENTROPY) return fail(h, -1, "%s confidence: unknown measure %d (0 prob, 1 entropy)", what, measure);
  if (agg < GAM_CF_MEAN || agg > GAM_CF_PROD) return fail(h, -1, "%s confidence: unknown aggregation %d (0 mean, 1 min, 2 prod)", what, agg);
  if (null_buf) return fail(h, -1, "%s confidence: NULL buffer", what);
  return 0;
}

static int ctc_conf_launch(gam_handle* h, const float* lp, const int32_t* enc_len, int B, int64_t Tp, int V, const int32_t* ids,
                           const int32_t* frames, const int32_t* counts, int cap, int measure, int agg, float* conf, int32_t* span,
                           int32_t* status, hipStream_t s) {
  if (int r = conf_shape_check(h, "CTC", B, Tp, V, cap, 1 << 24, measure, agg,
                               !lp || !enc_len || !counts || !status || (cap > 0 && (!ids || !frames || !conf || !span))))
    return r;
  const long rows = (long)B * Tp;
  if (int r = ensure(h, h->cf_stats, (size_t)rows * 2 + 64)) return r;
  const float inv_lnv = (float)(1.0 / std::log((double)V));
  {
    GamConfStatArgs a;
    a.lp = lp; a.enc_len = enc_len; a.stats = reinterpret_cast<int2*>(h->cf_stats.p); a.rows = (int)rows; a.Tp = (int)Tp; a.V = V;
    a.measure = measure; a.inv_lnv = inv_lnv;
    ProfScope ps(h, s, GAM_PF_DECODE, (double)rows * V * 4.0);
    if (V <= 64) hipLaunchKernelGGL(gam_ctc_conf_stats_kernel<16>, dim3(gam_cdiv(rows, 16)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(gam_ctc_conf_stats_kernel<64>, dim3(gam_cdiv(rows, 4)), dim3(256), 0, s, a);
    HIPCHK(h, hipGetLastError());
  }
  GamConfAggArgs a;
  a.lp = lp; a.stats = reinterpret_cast<const int2*>(h->cf_stats.p); a.enc_len = enc_len; a.ids = ids; a.frames = frames; a.counts = counts;
  a.Tp = (int)Tp; a.V = V; a.cap = cap; a.measure = measure; a.agg = agg; a.conf = conf; a.span = span; a.status = status;
  ProfScope ps(h, s, GAM_PF_DECODE, (double)rows * 8.0);
  hipLaunchKernelGGL(gam_ctc_conf_agg_kernel, dim3(B), dim3(256), 0, s, a);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int gam_ctc_confidence(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, const int32_t* ids,
                       const int32_t* frames, const int32_t* counts, int cap, int measure, int agg, float* conf, int32_t* span,
                       int32_t* status, void* stream) {
  if (int r = head_check(h, GAM_HEAD_CTC, "CTC head")) return r;
  GAM_DECODE_ENTRY(h, stream);
  const int V = h->cfg.num_classes;
  if (int r = conf_shape_check(h, "CTC", B, Tp, V, cap, 1 << 24, measure, agg, !encoded)) return r;
  if (int r = ctc_log_probs(h, encoded, B, Tp, nullptr, s)) return r;
  return ctc_conf_launch(h, h->logits.p, enc_len, B, Tp, V, ids, frames, counts, cap, measure, agg, conf, span, status, s);
}

int gam_op_ctc_confidence(gam_handle* h, const float* log_probs, const int32_t* enc_len, int B, int64_t Tp, int V, const int32_t* ids,
                          const int32_t* frames, const int32_t* counts, int cap, int measure, int agg, float* conf, int32_t* span,
                          int32_t* status, void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  return ctc_conf_launch(h, log_probs, enc_len, B, Tp, V, ids, frames, counts, cap, measure, agg, conf, span, status, s);
}

// ONE utterance of any length: memset (the validity word), check (validity over the token grid; T to the word beside it), the batch
// op's row pass with B = 1, the span walk over the token grid.  The workspace is cf_stats, as the batch op's: T x 8 bytes + the two words.
int gam_op_ctc_confidence_long(gam_handle* h, const float* log_probs, int64_t T, int V, const int32_t* ids, const int32_t* frames,
                               const int32_t* count, int cap, int measure, int agg, int wildcard, float* conf, int32_t* span,
                               int32_t* status, void* stream) {
  GAM_DECODE_ENTRY(h, stream);
  if (T < 1 || T > 2147483647ll || V < 2 || V > GAM_CF_MAX_V)
    return fail(h, -1, "long CTC confidence: bad shape T=%lld V=%d (1 <= T < 2^31, 2 <= V <= %d)", (long long)T, V, GAM_CF_MAX_V);
  if (cap < 0) return fail(h, -1, "long CTC confidence: cap=%d tokens is negative", cap);
  if (measure != GAM_CF_PROB && measure != GAM_CF_ENTROPY) return fail(h, -1, "long CTC confidence: unknown measure %d (0 prob, 1 entropy)", measure);
  if (agg < GAM_CF_MEAN || agg > GAM_CF_PROD) return fail(h, -1, "long CTC confidence: unknown aggregation %d (0 mean, 1 min, 2 prod)", agg);
  if (wildcard != 0 && wildcard != 1) return fail(h, -1, "long CTC confidence: wildcard=%d must be 0 or 1", wildcard);
  if (!log_probs || !count || !status || (cap > 0 && (!ids || !frames || !conf || !span))) return fail(h, -1, "long CTC confidence: NULL buffer");
  if (int r = ensure(h, h->cf_stats, (size_t)T * 2 + 64)) return r;
  GamConfLongArgs a;
  a.lp = log_probs; a.stats = reinterpret_cast<const int2*>(h->cf_stats.p); a.ctrl = h->cf_stats.as<int>() + (size_t)T * 2; a.ids = ids;
  a.frames = frames; a.count = count; a.T = (int)T; a.V = V; a.cap = cap; a.measure = measure; a.agg = agg; a.wildcard = wildcard;
  a.conf = conf; a.span = span; a.status = status;
  const unsigned tok_blocks = (unsigned)gam_cdiv(cap > 0 ? cap : 1, 256);
  HIPCHK(h, hipMemsetAsync(a.ctrl, 0, sizeof(int), s));
  hipLaunchKernelGGL(gam_ctc_conf_long_check_kernel, dim3(tok_blocks), dim3(256), 0, s, a);
  HIPCHK(h, hipGetLastError());
  {
    GamConfStatArgs sa;
    sa.lp = log_probs; sa.enc_len = a.ctrl + 1; sa.stats = reinterpret_cast<int2*>(h->cf_stats.p); sa.rows = (int)T; sa.Tp = (int)T; sa.V = V;
    sa.measure = measure; sa.inv_lnv = (float)(1.0 / std::log((double)V));
    ProfScope ps(h, s, GAM_PF_DECODE, (double)T * V * 4.0);
    if (V <= 64) hipLaunchKernelGGL(gam_ctc_conf_stats_kernel<16>, dim3((unsigned)((T + 15) / 16)), dim3(256), 0, s, sa);
    else hipLaunchKernelGGL(gam_ctc_conf_stats_kernel<64>, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, sa);
    HIPCHK(h, hipGetLastError());
  }
  ProfScope ps(h, s, GAM_PF_DECODE, (double)T * 8.0);
  hipLaunchKernelGGL(gam_ctc_conf_long_agg_kernel, dim3(tok_blocks), dim3(256), 0, s, a);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// From the encoder projection encp [B, Tp, JH]: the rows are checked, then the teacher-forced predictor and its projection (rnnt_tf_pp,
// the decoded ids as targets), then the joint at the listed nodes.
static int rnnt_conf_launch(gam_handle* h, const float* encp, const int32_t* enc_len, int B, int64_t Tp, const int32_t* ids,
                            const int32_t* frames, const int32_t* counts, int cap, int measure, float* conf, int32_t* status, hipStream_t s) {
  const gam_config& c = h->cfg;
  const int V = c.num_classes, H = c.pred_hidden, JH = c.joint_hidden, L = c.pred_rnn_layers;
  if (int r = conf_shape_check(h, "RNN-T", B, Tp, V, cap, GAM_RA_MAX_U, measure, GAM_CF_MEAN,
                               !encp || !enc_len || !counts || !status || (cap > 0 && (!ids || !frames || !conf))))
    return r;
  if (H > GAM_RA_MAX_H || JH > GAM_RA_MAX_H || H % 16 != 0 || JH % 16 != 0 || L < 1 || L > 4)
    return fail(h, -1, "RNN-T confidence: H=%d / JH=%d must be multiples of 16 up to %d, 1..4 predictor layers (L=%d)", H, JH, GAM_RA_MAX_H, L);
  {
    GamRnntConfPrepArgs a;
    a.enc_len = enc_len; a.ids = ids; a.frames = frames; a.counts = counts; a.Tp = (int)Tp; a.V = V; a.cap = cap; a.conf = conf; a.status = status;
    ProfScope ps(h, s, GAM_PF_DECODE, (double)B * cap * 12.0);
    hipLaunchKernelGGL(gam_rnnt_conf_prep_kernel, dim3(B), dim3(256), 0, s, a);
    HIPCHK(h, hipGetLastError());
  }
  if (cap == 0) return 0;
  if (int r = rnnt_tf_pp(h, ids, counts, B, cap, s)) return r;
  GamRnntConfArgs a;
  a.encp = encp; a.predp = h->ra_pp.p; a.ids = ids; a.frames = frames; a.counts = counts; a.status = status; a.wout = h->jn_out_w;
  a.bout = h->jn_out_b; a.conf = conf; a.Tp = (int)Tp; a.cap = cap; a.V = V; a.JH = JH; a.measure = measure;
  a.inv_lnv = (float)(1.0 / std::log((double)V));
  ProfScope ps(h, s, GAM_PF_DECODE, (double)B * cap * ((double)V * JH * 2.0));
  hipLaunchKernelGGL(gam_rnnt_conf_nodes_kernel, dim3(gam_cdiv(cap, 16), B), dim3(64), gam_cf_nodes_lds_bytes(JH), s, a);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int gam_rnnt_confidence(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, const int32_t* ids,
                        const int32_t* frames, const int32_t* counts, int cap, int measure, float* conf, int32_t* status, void* stream) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "RNN-T head")) return r;
  GAM_DECODE_ENTRY(h, stream);
  if (int r = conf_shape_check(h, "RNN-T", B, Tp, h->cfg.num_classes, cap, GAM_RA_MAX_U, measure, GAM_CF_MEAN, !encoded)) return r;
  if (int r = rnnt_encp(h, encoded, B, Tp, s)) return r;
  return rnnt_conf_launch(h, h->encp.p, enc_len, B, Tp, ids, frames, counts, cap, measure, conf, status, s);
}

int gam_op_rnnt_confidence(gam_handle* h, const float* encp, const int32_t* enc_len, int B, int64_t Tp, const int32_t* ids,
                           const int32_t* frames, const int32_t* counts, int cap, int measure, float* conf, int32_t* status, void* stream) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "RNN-T head")) return r;
  GAM_DECODE_ENTRY(h, stream);
  return rnnt_conf_launch(h, encp, enc_len, B, Tp, ids, frames, counts, cap, measure, conf, status, s);
}

int gam_rnnt_predict(gam_handle* h, const int32_t* labels, const float* h_in, const float* c_in, int B, float* g_out,
                     float* h_out, float* c_out, void* stream) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "gam_rnnt_predict")) return r;
  if (B <= 0 || !g_out || !h_out || !c_out || (h_in == nullptr) != (c_in == nullptr)) return fail(h, -1, "bad gam_rnnt_predict arguments");
  HIPCHK(h, hipSetDevice(h->device));
  const gam_config& c = h->cfg;
  GamPredictArgs a;
  rnnt_pred_weights(h, a);
  a.label = labels; a.h_in = h_in; a.c_in = c_in; a.g_out = g_out; a.h_out = h_out; a.c_out = c_out;
  a.B = B; a.PH = c.pred_hidden; a.V = c.num_classes; a.L = c.pred_rnn_layers;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(h, s, GAM_PF_DECODE, 0.0);
  hipLaunchKernelGGL(gam_rnnt_predict_kernel, dim3(B), dim3(256), (size_t)6 * c.pred_hidden * sizeof(float), s, a);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int gam_rnnt_joint(gam_handle* h, const float* enc, const float* dec, int B, int T, int U, float* log_probs, void* stream) {
  if (int r = head_check(h, GAM_HEAD_RNNT, "gam_rnnt_joint")) return r;
  if (B <= 0 || T <= 0 || U <= 0 || !enc || !dec || !log_probs) return fail(h, -1, "bad gam_rnnt_joint arguments");
  HIPCHK(h, hipSetDevice(h->device));
  const gam_config& c = h->cfg;
  const int D = c.d_model, PH = c.pred_hidden, JH = c.joint_hidden, V = c.num_classes;
  const size_t rows = (size_t)B * T * U;
  if (rows * std::max(JH, V) > ((size_t)1 << 31)) return fail(h, -1, "gam_rnnt_joint: B x T x U = %zu rows is too large for one call", rows);
  hipStream_t s = (hipStream_t)stream;
  DecodeScope ds(h, s);
  if (int r = ensure(h, h->encp, (size_t)B * T * JH)) return r;
  if (int r = ensure(h, h->jp, (size_t)B * U * JH)) return r;
  if (int r = ensure(h, h->jz, rows * JH)) return r;
  if (int r = ensure(h, h->jl, rows * V)) return r;
  // exact-fp32 MFMA GEMMs like the greedy path's projection (gemm() without split planes): enc [B T, D] and dec [B U, PH]
  GamGemmArgs ge = gemm_args(enc, D, h->jn_enc_w, h->jn_enc_b, h->encp.p, JH, B * T, JH, D);
  if (int r = gemm(h, s, ge, GAM_ACT_NONE, GAM_PF_DECODE)) return r;
  GamGemmArgs gp = gemm_args(dec, PH, h->jn_pred_w, h->jn_pred_b, h->jp.p, JH, B * U, JH, PH);
  if (int r = gemm(h, s, gp, GAM_ACT_NONE, GAM_PF_DECODE)) return r;
  {
    ProfScope ps(h, s, GAM_PF_DECODE, (double)rows * JH * 4.0);
    const int grid = (int)std::min<size_t>((rows * JH + 255) / 256, 8192);
    hipLaunchKernelGGL(gam_joint_hidden_kernel, dim3(grid), dim3(256), 0, s, h->encp.p, h->jp.p, h->jz.p, B, T, U, JH);
    HIPCHK(h, hipGetLastError());
  }
  GamGemmArgs go = gemm_args(h->jz.p, JH, h->jn_out_w, h->jn_out_b, h->jl.p, V, (int)rows, V, JH);
  if (int r = gemm(h, s, go, GAM_ACT_NONE, GAM_PF_DECODE)) return r;
  ProfScope ps(h, s, GAM_PF_DECODE, (double)rows * V * 8.0);
  hipLaunchKernelGGL(gam_log_softmax_kernel, dim3(gam_cdiv((long)rows, 4)), dim3(256), 0, s, h->jl.p, log_probs, (int)rows, V);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int gam_emo_probs(gam_handle* h, const float* encoded, const int32_t* enc_len, int B, int64_t Tp, float* probs,
                  void* stream) {
  if (int r = head_check(h, GAM_HEAD_EMO, nullptr)) return r;   // (no finalize message of its own: has_head is set at gam_finalize)
  if (B <= 0 || Tp <= 0 || !encoded || !probs) return fail(h, -1, "bad emotion-head arguments");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const int D = h->cfg.d_model, NC = h->cfg.num_classes;
  ProfScope ps(h, s, GAM_PF_DECODE, (double)B * D * Tp * 4.0);
  hipLaunchKernelGGL(gam_emo_head_kernel, dim3(B), dim3(256), (size_t)(D + NC) * sizeof(float), s, encoded, enc_len,
                     h->emo_w, h->emo_b, probs, D, (int)Tp, NC);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int gam_op_gemm(gam_handle* h, const float* A, const float* W, const float* bias, float* C, int M, int N, int K, int act,
                void* stream) {
  return gam_op_gemm_ex(h, A, W, bias, nullptr, 1.0f, C, M, N, K, act, stream);
}

static int op_gemm_impl(gam_handle* h, const float* A, const float* W, const float* bias, const float* R, float alpha, float* C, long ldc,
                        int M, int N, int K, int act, int c_split, int c_guard, void* stream);

int gam_op_gemm_ex(gam_handle* h, const float* A, const float* W, const float* bias, const float* R, float alpha, float* C, int M,
                   int N, int K, int act, void* stream) {
  if (!h) return -1;
  return op_gemm_impl(h, A, W, bias, R, alpha, C, N, M, N, K, act, 0, 0, stream);
}

int gam_op_gemm_fmt(gam_handle* h, const float* A, const float* W, const float* bias, const float* R, float alpha, float* C, int64_t ldc,
                    int M, int N, int K, int act, int c_split, int c_guard, void* stream) {
  if (!h) return -1;
  if (!split_mode(h) || K % 32 != 0 || N % 4 != 0 || ldc < N || c_split < 0 || c_split > 2 || (c_split == 1 && ldc % 32 != 0) ||
      (c_split == 2 && !(h->gemm_mode == GAM_GEMM_F16 && K % 64 == 0)))
    return fail(h, -1, "gam_op_gemm_fmt: format %d / pitch %ld not available for this mode and shape (N=%d K=%d)", c_split, (long)ldc, N, K);
  return op_gemm_impl(h, A, W, bias, R, alpha, C, (long)ldc, M, N, K, act, c_split, c_guard, stream);
}

static int op_gemm_impl(gam_handle* h, const float* A, const float* W, const float* bias, const float* R, float alpha, float* C, long ldc,
                        int M, int N, int K, int act, int c_split, int c_guard, void* stream) {
  HIPCHK(h, hipSetDevice(h->device));
  GamGemmArgs g = gemm_args(A, K, W, bias, C, ldc, M, N, K);
  g.R = R; g.ldr = ldc; g.alpha = alpha;
  g.c_split = c_split; g.c_guard = c_guard;
  hipStream_t s = (hipStream_t)stream;
  // the exact-fp32 kernel: the exact mode, and the shapes the LDS-DMA kernel cannot take (its epilogue moves 4-column pieces)
  if (!split_mode(h) || K % 32 != 0 || N % 4 != 0) return gemm(h, s, g, act);
  // split-fp16 modes: both operands converted by pre-passes on every call (in the encoder the producing kernels write sp32
  // directly and the weight planes are built at gam_finalize) -- a cache keyed on the W pointer returned stale planes when an
  // allocator handed the same address to a new matrix of the same size.  This is a test / microbenchmark entry; the HIP-event
  // profile class times only the GEMM launch, not these conversions.
  const size_t wn = (size_t)N * K, an = (size_t)M * K;
  W16 w16;   // unit scale
  if (int r = ensure(h, h->op_sp, wn + 64)) return r;
  hipLaunchKernelGGL(gam_to_sp32_kernel, dim3((int)std::min<size_t>((wn / 4 + 255) / 256, 4096)), dim3(256), 0, s, W,
                     (_Float16*)h->op_sp.p, wn / 4, (const float*)nullptr, K);
  w16.sp = (_Float16*)h->op_sp.p;
  // per-row power-of-two scale of A, as the LayerNorm kernels provide it inside the encoder
  if (int r = ensure(h, h->op_rs, (size_t)M + 64)) return r;
  hipLaunchKernelGGL(gam_rowscale_kernel, dim3(gam_cdiv(M, 4)), dim3(256), 0, s, A, h->op_rs.p, M, K, (long)K);
  g.a_rs = h->op_rs.p;
  if (int r = ensure(h, h->aplanes, an + 64)) return r;
  g.Asp = (const _Float16*)h->aplanes.p;
  g.a_fmt = (h->gemm_mode == GAM_GEMM_F16 && K % 64 == 0) ? 2 : 1;   // (other K: the three-term kernel, whatever the mode)
  if (g.a_fmt == 2) {
    if (int r = ensure(h, h->op_planes, wn / 2 + 64)) return r;
    w16.h16 = (_Float16*)h->op_planes.p;
    hipLaunchKernelGGL(gam_to_h16_kernel, dim3((int)std::min<size_t>((wn / 4 + 255) / 256, 4096)), dim3(256), 0, s, W, w16.h16,
                       wn / 4, (const float*)nullptr, K);
    hipLaunchKernelGGL(gam_to_h16_kernel, dim3((int)std::min<size_t>((an / 4 + 255) / 256, 8192)), dim3(256), 0, s, A,
                       (_Float16*)h->aplanes.p, an / 4, (const float*)h->op_rs.p, K);
  } else {
    hipLaunchKernelGGL(gam_to_sp32_kernel, dim3((int)std::min<size_t>((an / 4 + 255) / 256, 8192)), dim3(256), 0, s, A,
                       (_Float16*)h->aplanes.p, an / 4, (const float*)h->op_rs.p, K);
  }
  return gemm(h, s, g, act, GAM_PF_GEMM, &w16);
}

int gam_op_attention(gam_handle* h, const float* q, const float* k, const float* v, float* ctx, const int32_t* lens, int B,
                     int T, int H, void* stream) {
  if (!h) return -1;
  if (B <= 0 || T <= 0 || H <= 0) return fail(h, -1, "bad attention shape");
  HIPCHK(h, hipSetDevice(h->device));
  return launch_attention(h, (hipStream_t)stream, q, k, v, H * GAM_ATT_DK, ctx, 0, lens, nullptr, B, T, T, H, nullptr, nullptr, nullptr);
}

int gam_op_attention_ex(gam_handle* h, const float* q, const float* k, const float* v, int64_t ldq, float* ctx, const int32_t* lens,
                        const int32_t* cu, int B, int Ta, int Tv, int H, const float* pbuf, const float* pos_u, const float* pos_v,
                        void* stream) {
  if (!h) return -1;
  const int D = H * GAM_ATT_DK;
  if (B <= 0 || Ta <= 0 || Tv <= 0 || H <= 0) return fail(h, -1, "bad attention shape");
  if (cu == nullptr && Tv > Ta) return fail(h, -1, "attention: Tv %d > Ta %d in the padded layout", Tv, Ta);
  if (ldq < D || ldq % 4 != 0) return fail(h, -1, "attention: row stride %ld (H*48 = %d, multiple of 4)", (long)ldq, D);
  if (pbuf != nullptr && (pos_u == nullptr || pos_v == nullptr)) return fail(h, -1, "attention: pbuf without pos_u / pos_v");
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };   // (float4 loads and stores)
  if (!al16(q) || !al16(k) || !al16(v) || !al16(ctx) || (pbuf && (!al16(pbuf) || !al16(pos_u) || !al16(pos_v))))
    return fail(h, -1, "attention: operands must be 16-byte aligned");
  HIPCHK(h, hipSetDevice(h->device));
  return launch_attention(h, (hipStream_t)stream, q, k, v, (long)ldq, ctx, 0, lens, cu, B, Ta, Tv, H, pbuf, pos_u, pos_v);
}

int gam_op_layernorm(gam_handle* h, const gam_ln_op* op, void* stream) {
  if (!h) return -1;
  if (!op) return fail(h, -1, "layernorm: null argument block");
  const gam_ln_op& o = *op;
  if (o.mode < 0 || o.mode > 2) return fail(h, -1, "layernorm: mode %d outside 0..2", o.mode);
  if (o.rows <= 0 || o.d <= 0) return fail(h, -1, "layernorm: bad shape rows %d d %d", o.rows, o.d);
  if (o.split1 < 0 || o.split1 > 2 || o.split2 < 0 || o.split2 > 2)
    return fail(h, -1, "layernorm: store format %d / %d outside 0..2", o.split1, o.split2);
  if (!o.out1 || !o.w1 || !o.b1) return fail(h, -1, "layernorm: out1 / w1 / b1 are mandatory");
  if (!o.part && !o.x) return fail(h, -1, "layernorm: x is mandatory without part");
  if (o.part && o.mode != 2 && !o.xstore) return fail(h, -1, "layernorm: part without xstore");
  if (o.mode != 0 && !o.out2) return fail(h, -1, "layernorm: mode %d needs out2", o.mode);
  if (o.mode == 2 && (!o.w2 || !o.b2)) return fail(h, -1, "layernorm: mode 2 needs w2 / b2");
  if (o.mode == 1) {
    if (!o.rcos || !o.rsin || o.rope_rows <= 0) return fail(h, -1, "layernorm: mode 1 needs rcos / rsin of rope_rows > 0 rows");
    if (o.dk <= 0) return fail(h, -1, "layernorm: mode 1 needs dk > 0");
    if (!o.row_t && o.ta <= 0) return fail(h, -1, "layernorm: mode 1 needs row_t or ta > 0");
  }
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };   // (float4 loads and stores; null passes)
  if (!al16(o.x) || !al16(o.out1) || !al16(o.out2) || !al16(o.w1) || !al16(o.b1) || !al16(o.w2) || !al16(o.b2) || !al16(o.rcos) ||
      !al16(o.rsin) || !al16(o.part) || !al16(o.pbias) || !al16(o.presid) || !al16(o.xstore))
    return fail(h, -1, "layernorm: operands must be 16-byte aligned");
  HIPCHK(h, hipSetDevice(h->device));
  GamLnArgs a;
  memset(&a, 0, sizeof a);
  a.x = o.x; a.out1 = o.out1; a.out2 = o.out2; a.w1 = o.w1; a.b1 = o.b1; a.w2 = o.w2; a.b2 = o.b2;
  a.rcos = o.rcos; a.rsin = o.rsin; a.rows = o.rows; a.d = o.d; a.ta = o.ta; a.dk = o.dk; a.eps = o.eps;
  a.split1 = o.split1; a.split2 = o.split2; a.rs = o.rs; a.rope_rows = o.rope_rows;
  a.part = o.part; a.nsplit = o.nsplit; a.pbias = o.pbias; a.presid = o.presid; a.palpha = o.palpha; a.xstore = o.xstore;
  a.row_t = o.row_t;
  hipError_t e = gam_launch_layernorm(a, o.mode, (hipStream_t)stream);
  if (e != hipSuccess)
    return fail(h, -2, "layernorm launch (mode %d, rows %d, d %d, dk %d, split %d/%d, nsplit %d): %s", o.mode, o.rows, o.d, o.dk,
                o.split1, o.split2, o.part ? o.nsplit : 0, hipGetErrorString(e));
  return 0;
}

int gam_op_convmod(gam_handle* h, const float* u, float* z, const float* dw_w, const float* dw_b, const float* n_scale,
                   const float* n_shift, const int32_t* lens, const int32_t* cu, int B, int Ta, int Tv, int d, int ks, int layer_norm,
                   int z_split, void* stream) {
  if (!h) return -1;
  if (!h->finalized) return fail(h, -1, "gam_op_convmod before gam_finalize");   // (the range flag is allocated there)
  if (!u || !z || !dw_w || !dw_b || !n_scale || !n_shift || !lens) return fail(h, -1, "conv module: null operand");
  if (B <= 0 || Ta <= 0 || Tv <= 0 || d <= 0) return fail(h, -1, "conv module: bad shape B %d Ta %d Tv %d d %d", B, Ta, Tv, d);
  if (cu == nullptr && Tv > Ta) return fail(h, -1, "conv module: Tv %d > Ta %d in the padded layout", Tv, Ta);
  if (z_split < 0 || z_split > 2) return fail(h, -1, "conv module: store format %d outside 0..2", z_split);
  if (z_split && d % 32 != 0) return fail(h, -1, "conv module: a split-fp16 z needs d %% 32 == 0 (d = %d)", d);
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  // the BatchNorm kernel and the 4-channel LayerNorm kernel move f32x4; the element-wise LayerNorm kernel (d % 4 != 0) does not
  if (d % 4 == 0 && (!al16(u) || !al16(z) || !al16(dw_b) || !al16(n_scale) || !al16(n_shift)))
    return fail(h, -1, "conv module: operands must be 16-byte aligned");
  HIPCHK(h, hipSetDevice(h->device));
  hipError_t e = launch_convmod(h, (hipStream_t)stream, u, z, dw_w, dw_b, n_scale, n_shift, lens, cu, B, Ta, Tv, d, ks, layer_norm != 0, z_split);
  if (e != hipSuccess) return fail(h, -2, "conv-module launch (k=%d, d=%d, %s): %s", ks, d, layer_norm ? "LayerNorm" : "BatchNorm", hipGetErrorString(e));
  return 0;
}

int gam_set_gemm_mode(gam_handle* h, int mode) {
  if (!h || (mode != GAM_GEMM_F32 && mode != GAM_GEMM_F16X3 && mode != GAM_GEMM_F16)) return fail(h, -1, "unknown GEMM mode %d", mode);
  h->gemm_mode = mode;
  return 0;
}

int gam_get_gemm_mode(const gam_handle* h) { return h ? h->gemm_mode : -1; }

// Debug: FNV-1a hash of one of the decode's scratch buffers as it is in device memory now (the call synchronises the device).
// which: 0 = token-major encoder output (tok), 1 = encoder projection (encp), 2 = hand-off granules (rnnt_x), 3 = CTC logits.
int gam_debug_buffer_hash(gam_handle* h, int which, uint64_t* hash_out, int64_t* floats_out) {
  if (!h || !hash_out) return -1;
  const DevBuf* b = which == 0 ? &h->tok : which == 1 ? &h->encp : which == 2 ? &h->rnnt_x : which == 3 ? &h->logits : nullptr;
  if (!b) return fail(h, -1, "no such buffer %d", which);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipDeviceSynchronize());
  std::vector<uint32_t> host(b->cap);
  if (b->cap) HIPCHK(h, hipMemcpy(host.data(), b->p, b->cap * sizeof(float), hipMemcpyDeviceToHost));
  uint64_t x = 1469598103934665603ull;
  for (uint32_t v : host) { x ^= v; x *= 1099511628211ull; }
  *hash_out = x;
  if (floats_out) *floats_out = (int64_t)b->cap;
  return 0;
}

int gam_set_rnnt_cluster(gam_handle* h, int workgroups_per_utterance) {
  if (!h) return -1;
  if (workgroups_per_utterance < -1 || workgroups_per_utterance > 8) return fail(h, -1, "cluster size %d outside -1 (auto) .. 8", workgroups_per_utterance);
  h->rnnt_cluster = workgroups_per_utterance;
  return 0;
}

int gam_get_rnnt_cluster(gam_handle* h) { return h ? h->rnnt_cluster : -2; }

int gam_rnnt_cluster_plan_info(int ncu, int cluster, int exclusive, int B, int H, int JH, int V, int L, int32_t* out) {
  if (!out || B <= 0 || H <= 0 || JH <= 0 || V <= 0 || L <= 0) return -1;
  const RnntClusterPlan p = rnnt_cluster_plan(ncu, cluster, exclusive, B, H, JH, V, L);
  memset(out, 0, 8 * sizeof(int32_t));
  if (p.C == 0) return 0;
  out[0] = p.C; out[1] = p.nr; out[2] = p.kern; out[3] = p.resident ? 1 : 0;
  out[4] = p.wout_slice_in_lds; out[5] = p.wpred_slice_in_lds; out[6] = (int32_t)p.lds; out[7] = (int32_t)p.grid;
  return 0;
}

int gam_rnnt_last_decode(gam_handle* h, int32_t* out) {
  if (!h || !out) return -1;
  out[0] = h->last_rnnt_c; out[1] = h->last_rnnt_kern; out[2] = h->last_rnnt_refused;
  return 0;
}

int gam_last_encode_rows(gam_handle* h, int* rows_padded) {
  if (!h) return -1;
  if (rows_padded) *rows_padded = h->last_rows_padded;
  return h->last_rows;
}

int gam_range_flag(gam_handle* h, int* flag_host, void* stream) {
  if (!h || !flag_host) return -1;
  if (!h->finalized) return fail(h, -1, "gam_range_flag before gam_finalize");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(h, hipMemcpyAsync(flag_host, h->range_flag, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemsetAsync(h->range_flag, 0, sizeof(int), s));
  HIPCHK(h, hipStreamSynchronize(s));
  return 0;
}

int gam_range_flag_fetch(gam_handle* h, int32_t* flag_dev, void* stream) {
  if (!h || !flag_dev) return -1;
  if (!h->finalized) return fail(h, -1, "gam_range_flag_fetch before gam_finalize");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(h, hipMemcpyAsync(flag_dev, h->range_flag, sizeof(int), hipMemcpyDeviceToDevice, s));
  HIPCHK(h, hipMemsetAsync(h->range_flag, 0, sizeof(int), s));
  return 0;
}

int gam_plan_sp(int M, int N, int K, int n_cu, int* mt, int* nw, int* splitk) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 32 != 0 || !mt || !nw || !splitk) return -1;
  const GamSpPlan p = gam_gemm_sp_plan(M, N, K, 0, n_cu > 0 ? n_cu : 256);
  *mt = p.mt; *nw = p.nw; *splitk = p.s;
  return 0;
}

int gam_tune_sp(int mt, int nw, int splitk) {
  GamSpForce& f = gam_sp_force();
  f.mt = mt; f.nw = nw; f.s = splitk;
  return 0;
}

int gam_tune_sp_stages(int stages) {
  if (stages != 0 && stages != 2 && stages != 3) return -1;
  gam_sp_force().ns = stages;
  return 0;
}

int gam_plan_sp_ex(int M, int N, int K, int n_cu, int* mt, int* nw, int* splitk, int* stages) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 32 != 0 || !mt || !nw || !splitk || !stages) return -1;
  const GamSpPlan p = gam_gemm_sp_plan(M, N, K, 0, n_cu > 0 ? n_cu : 256);
  *mt = p.mt; *nw = p.nw; *splitk = p.s; *stages = p.ns;
  return 0;
}

int gam_resample_plan(int rate_in, int rate_out, int* up, int* down, int* taps) {
  GamRsPlan p;
  const int rc = gam_rs_plan(rate_in, rate_out, &p);
  if (rc != 0) return rc;
  if (up) *up = (int)p.N;
  if (down) *down = (int)p.O;
  if (taps) *taps = p.K;
  return 0;
}

int gam_resample_tile(int rate_in, int rate_out, int* tile, int* form) {
  GamRsPlan p;
  const int rc = gam_rs_plan(rate_in, rate_out, &p);
  if (rc != 0) return rc;
  if (tile) *tile = p.tile;
  if (form) *form = p.form;
  return 0;
}

int gam_resample_table(int rate_in, int rate_out, float* coeff, int32_t* first) {
  GamRsPlan p;
  const int rc = gam_rs_plan(rate_in, rate_out, &p);
  if (rc != 0) return rc;
  if (!coeff || !first) return -1;
  gam_rs_table(p, coeff, first);
  return 0;
}

int64_t gam_resample_out_len(int rate_in, int rate_out, int64_t n_in) {
  GamRsPlan p;
  if (gam_rs_plan(rate_in, rate_out, &p) != 0) return -1;
  return gam_rs_out_len(p, n_in);
}

int gam_op_resample(const void* src, int fmt, int channels, int channel, const int64_t* len_in, int B, int64_t frames, int rate_in, int rate_out,
                    const float* coeff, const int32_t* first, float* dst, int64_t L_out, int64_t* len_out, void* stream) {
  return gam_rs_run(src, fmt, channels, channel, len_in, B, frames, rate_in, rate_out, coeff, first, dst, L_out, len_out, (hipStream_t)stream);
}

int gam_profile_enable(gam_handle* h, int on) {
  if (!h) return -1;
  h->prof_on = on;
  h->prof_used = 0;
  for (int i = 0; i < GAM_PF_NCLASS; ++i) { h->prof_work[i] = 0; h->prof_launches[i] = 0; h->prof_bytes[i] = 0; }
  return 0;
}

int gam_profile_pause(gam_handle* h, int on) {
  if (!h) return -1;
  h->prof_on = on;      // (no reset: what was collected so far stays)
  return 0;
}

int gam_profile_read_bytes(gam_handle* h, int cls, double* bytes) {
  if (!h || cls < 0 || cls >= GAM_PF_NCLASS || !bytes) return -1;
  *bytes = h->prof_bytes[cls];
  return 0;
}

int gam_profile_read(gam_handle* h, int cls, double* ms, int64_t* launches, double* work) {
  if (!h || cls < 0 || cls >= GAM_PF_NCLASS) return -1;
  double tot = 0;
  for (size_t i = 0; i < h->prof_used; ++i) {
    ProfEvent& e = h->prof_events[i];
    if (e.cls != cls) continue;
    HIPCHK(h, hipEventSynchronize(e.b));
    float t = 0;
    HIPCHK(h, hipEventElapsedTime(&t, e.a, e.b));
    tot += t;
  }
  if (ms) *ms = tot;
  if (launches) *launches = h->prof_launches[cls];
  if (work) *work = h->prof_work[cls];
  return 0;
}

}  // extern "C"
