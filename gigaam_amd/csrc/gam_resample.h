// gam_resample.h -- the stage before gam_frontend: raw interleaved audio frames -> mono fp32 at the model's rate.
//   reference: gigaam/preprocess.py:12-40 pipes every file through an ffmpeg subprocess (decode, downmix, resample to 16 kHz, 16-bit);
//   this is the same job on the GPU, defined as torchaudio.functional.resample defines it (sinc_interp_hann, lowpass_filter_width 6,
//   rolloff 0.99) because that definition is public, closed-form and checkable in fp64 (tests/resample_ref.py).
//
// With g = gcd(r_in, r_out), O = r_in / g, N = r_out / g, f = 0.99 min(O, N), L = 6 and x[m] = 0 outside [0, n_in):
//     y[j] = (f / O) sum_m x[m] sinc(pi t) cos^2(pi t / (2 L)),   t = f (m / O - j / N),   over the m with |t| < L.
// The terms depend on j only through p = j mod N, and the support is m in (j O / N - c, j O / N + c) with c = L O / f, so the filter is a
// table of N rows of K coefficients, and output j = q N + p reads x[base(j) + k], k < K, with base(j) = first[p] + q O = floor(j O / N - c) + 1
// (monotone in j).  Only this support is computed (torchaudio's 2 width + O taps per phase are mostly zeros).  Equal rates are the
// identity (one tap of 1.0), as in torchaudio.  All the integer arithmetic of the plan is exact (128-bit where a product needs it).
//
// Kernel: a workgroup owns `tile` consecutive outputs of one row.  It stages, into LDS, the input span the tile reads -- converted to fp32
// and downmixed while staging, four independent loads per thread in flight -- and the coefficient rows of the tile's phases (all N rows
// once tile >= N) at an odd row pitch, then each thread forms its outputs as K fp32 FMAs in tap order, up to four outputs side by side.
// With N = 1 there is one coefficient row: every lane reads the same coefficient, so it comes through the scalar cache instead of LDS.
// The host sizes the tile so that span and rows fit GAM_RS_SPAN / GAM_RS_TABLE.  Measured: one hour of 48 kHz stereo
// PCM16 in 0.25 ms, 3.7 TB/s over input + output bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

enum { GAM_RS_U8 = 0, GAM_RS_I16 = 1, GAM_RS_I24 = 2, GAM_RS_I32 = 3, GAM_RS_F32 = 4, GAM_RS_MULAW = 5, GAM_RS_ALAW = 6, GAM_RS_NFMT = 7 };
// kernel forms (gam_resample_tile reports the one a rate pair gets)
enum { GAM_RS_FORM_SINGLE = 0,   // N = 1: one coefficient row, read lane-uniformly
       GAM_RS_FORM_TABLE = 1,    // N > 1, tile >= N: the whole table in LDS
       GAM_RS_FORM_ROWS = 2 };   // N > 1, tile < N: the tile's own rows in LDS (a table too large for LDS, or a span that caps the tile)

constexpr int GAM_RS_MAX_RATE = 384000;
constexpr int64_t GAM_RS_MAX_TABLE = 1 << 18;     // N K entries
constexpr int GAM_RS_WIDTH = 6;                   // L: zero crossings on each side
constexpr int GAM_RS_THREADS = 256;
constexpr int GAM_RS_TILE_MAX = 2048;
// LDS budget in 4-byte words: span + rows * (pitch + 1) <= 4608 + 8960 = 54272 bytes, three workgroups per CU.  8960 words hold the
// largest table of the usual rates whole (11.025 k -> 16 k: 640 rows of 13 + 1).
constexpr int GAM_RS_SPAN = 4608;
constexpr int GAM_RS_TABLE = 8960;

struct GamRsPlan {
  int64_t O = 1, N = 1;   // input / output samples per period
  int K = 1;              // taps per output
  int tile = 1, form = GAM_RS_FORM_SINGLE, rows = 1, pitch = 1, span = 1;   // launch shape: outputs per workgroup, coefficient rows and row pitch in LDS, staged inputs
};

static inline int64_t gam_rs_gcd(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }
static inline int64_t gam_rs_floor_div(__int128 a, __int128 b) {   // b > 0
  __int128 q = a / b;
  if (a % b != 0 && a < 0) --q;
  return (int64_t)q;
}

// base(j) = floor(j O / N - c) + 1 and the last tap's input last(j) = ceil(j O / N + c) - 1, c = L O / f = 100 L O / (99 min(O, N))
static inline int64_t gam_rs_first(int64_t j, int64_t O, int64_t N) {
  const __int128 mn = O < N ? O : N, den = (__int128)99 * mn * N;
  return gam_rs_floor_div((__int128)99 * mn * j * O - (__int128)100 * GAM_RS_WIDTH * O * N, den) + 1;
}
static inline int64_t gam_rs_last(int64_t j, int64_t O, int64_t N) {
  const __int128 mn = O < N ? O : N, den = (__int128)99 * mn * N;
  return -gam_rs_floor_div(-((__int128)99 * mn * j * O + (__int128)100 * GAM_RS_WIDTH * O * N), den) - 1;
}

// 0 = ok, -1 = a rate outside 1..GAM_RS_MAX_RATE, -2 = table over GAM_RS_MAX_TABLE entries (or a filter longer than the LDS span)
static inline int gam_rs_plan(int rate_in, int rate_out, GamRsPlan* out) {
  if (rate_in < 1 || rate_in > GAM_RS_MAX_RATE || rate_out < 1 || rate_out > GAM_RS_MAX_RATE) return -1;
  GamRsPlan p;
  if (rate_in != rate_out) {
    const int64_t g = gam_rs_gcd(rate_in, rate_out);
    p.O = rate_in / g;
    p.N = rate_out / g;
    // every row has floor(2 c) or floor(2 c) + 1 taps: refuse before walking N rows of a table that cannot be accepted
    const int64_t mn = p.O < p.N ? p.O : p.N;
    if (p.N * (200 * GAM_RS_WIDTH * p.O / (99 * mn)) > GAM_RS_MAX_TABLE) return -2;
    int K = 0;
    for (int64_t ph = 0; ph < p.N; ++ph) {
      const int n = (int)(gam_rs_last(ph, p.O, p.N) - gam_rs_first(ph, p.O, p.N) + 1);
      K = n > K ? n : K;
    }
    p.K = K;
    if (p.N * K > GAM_RS_MAX_TABLE || K + 2 >= GAM_RS_SPAN) return -2;
  }
  // the tile: as many outputs as keep the span (tile - 1) O / N + 2 + K inside the LDS budget
  p.pitch = p.K | 1;          // odd: lanes on consecutive rows fall on different LDS banks
  int64_t tile = (int64_t)(GAM_RS_SPAN - p.K - 2) * p.N / p.O;
  tile = tile > GAM_RS_TILE_MAX ? GAM_RS_TILE_MAX : tile;
  if (p.N > 1) {
    const int64_t fit = GAM_RS_TABLE / (p.pitch + 1);
    if (p.N > fit || tile < p.N) tile = tile < fit ? tile : fit;
  }
  if (tile >= GAM_RS_THREADS) tile -= tile % GAM_RS_THREADS;
  if (tile < 1) return -2;
  p.tile = (int)tile;
  p.form = p.N == 1 ? GAM_RS_FORM_SINGLE : (tile >= p.N ? GAM_RS_FORM_TABLE : GAM_RS_FORM_ROWS);
  p.rows = (int)(tile < p.N ? tile : p.N);
  p.span = (int)((tile - 1) * p.O / p.N) + 2 + p.K;
  *out = p;
  return 0;
}

static inline int64_t gam_rs_out_len(const GamRsPlan& p, int64_t n_in) { return n_in <= 0 ? 0 : (p.N * n_in + p.O - 1) / p.O; }

// the table in fp64, rounded to fp32: coeff [N, K] (taps beyond a row's support are zeros), first [N]
static inline void gam_rs_table(const GamRsPlan& p, float* coeff, int32_t* first) {
  if (p.O == p.N) { coeff[0] = 1.0f; first[0] = 0; return; }
  const double pi = 3.14159265358979323846, L = GAM_RS_WIDTH;
  const double f = 0.99 * (double)(p.O < p.N ? p.O : p.N);
  for (int64_t ph = 0; ph < p.N; ++ph) {
    const int64_t m0 = gam_rs_first(ph, p.O, p.N);
    first[ph] = (int32_t)m0;
    for (int k = 0; k < p.K; ++k) {
      const double t = f * (double)((m0 + k) * p.N - ph * p.O) / (double)(p.O * p.N);
      double c = 0.0;
      if (std::fabs(t) < L) {
        const double w = std::cos(pi * t / (2.0 * L));
        c = (f / (double)p.O) * (t == 0.0 ? 1.0 : std::sin(pi * t) / (pi * t)) * w * w;
      }
      coeff[ph * p.K + k] = (float)c;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ device
__device__ __forceinline__ int gam_rs_mulaw(unsigned b) {
  const unsigned u = ~b & 0xFFu;
  const int mag = ((int)(((u & 15u) << 3) + 0x84u) << ((u >> 4) & 7u)) - 0x84;
  return (u & 0x80u) ? -mag : mag;
}
__device__ __forceinline__ int gam_rs_alaw(unsigned b) {
  const unsigned a = (b ^ 0x55u) & 0xFFu, e = (a >> 4) & 7u, m = a & 15u;
  const int mag = e ? (int)(((m << 4) + 0x108u) << (e - 1u)) : (int)((m << 4) + 8u);
  return (a & 0x80u) ? mag : -mag;
}

// sample s (frame * channels + channel) of a row, as fp32 in [-1, 1)
template <int FMT>
__device__ __forceinline__ float gam_rs_sample(const unsigned char* __restrict__ row, int64_t s) {
  if (FMT == GAM_RS_U8) return (float)((int)row[s] - 128) * (1.0f / 128.0f);
  if (FMT == GAM_RS_I16) return (float)reinterpret_cast<const int16_t*>(row)[s] * (1.0f / 32768.0f);
  if (FMT == GAM_RS_I24) {   // bytewise: neither rows nor frames are 4-byte aligned
    const unsigned char* q = row + 3 * s;
    const int v = (int)((unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)(int)(signed char)q[2] << 16));
    return (float)v * (1.0f / 8388608.0f);
  }
  if (FMT == GAM_RS_I32) return (float)reinterpret_cast<const int32_t*>(row)[s] * (1.0f / 2147483648.0f);
  if (FMT == GAM_RS_F32) return reinterpret_cast<const float*>(row)[s];
  if (FMT == GAM_RS_MULAW) return (float)gam_rs_mulaw(row[s]) * (1.0f / 32768.0f);
  return (float)gam_rs_alaw(row[s]) * (1.0f / 32768.0f);
}

// frame m of a row as the mean of its channels: an fp32 sum in channel order times 1.0f / C
template <int FMT>
__device__ __forceinline__ float gam_rs_mean(const unsigned char* __restrict__ row, int64_t m, int channels, float inv_c) {
  float s = gam_rs_sample<FMT>(row, m * channels);
  for (int c = 1; c < channels; ++c) s += gam_rs_sample<FMT>(row, m * channels + c);
  return s * inv_c;
}

// xs[i] = frame m_lo + i of the row for i < n_span, zeros outside [0, n_in).  MODE 1: one channel; 2: the mean of two; 0: of `channels`.
// Four frames per thread are loaded before the first is used, from addresses clamped into the row (n_in >= 1), so that the loads of a
// thread do not wait for each other: a workgroup's time is the latency of its staging loads.
template <int FMT, int MODE>
__device__ __forceinline__ void gam_rs_stage(float* xs, const unsigned char* __restrict__ row, int64_t m_lo, int n_span, int64_t n_in,
                                             int channels, int channel, float inv_c) {
  for (int i0 = threadIdx.x; i0 < n_span; i0 += 4 * GAM_RS_THREADS) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int64_t m = m_lo + i0 + u * GAM_RS_THREADS;
      m = m < 0 ? 0 : (m >= n_in ? n_in - 1 : m);
      if (MODE == 1) v[u] = gam_rs_sample<FMT>(row, m * channels + channel);
      else if (MODE == 2) v[u] = (gam_rs_sample<FMT>(row, 2 * m) + gam_rs_sample<FMT>(row, 2 * m + 1)) * inv_c;
      else v[u] = gam_rs_mean<FMT>(row, m, channels, inv_c);
    }
    // (keeps the compiler from sinking each load into the branch that stores its value, where it would wait for it alone)
    asm volatile("" ::"v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]));
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * GAM_RS_THREADS;
      const int64_t m = m_lo + i;
      if (i < n_span) xs[i] = (m >= 0 && m < n_in) ? v[u] : 0.0f;
    }
  }
}

// what a thread needs to form outputs of its workgroup's tile; xs / ts / fs as word offsets into the workgroup's LDS
struct GamRsTile {
  const float* coeff; float* out;
  int ts, fs, O, N, K, pitch, cnt, cnt_all;
};

// outputs d0, d0 + 256, .. (G of them) of the tile: K FMAs each, in tap order, the G chains side by side.  An output behind the row's end
// (d >= cnt) is zero, one behind the buffer's (d >= cnt_all) is not written; both read tap 0's inputs so that no address leaves the span.
template <int G, bool SINGLE>
__device__ __forceinline__ void gam_rs_outputs(const GamRsTile& tl, int d0) {
  extern __shared__ float gam_rs_smem[];
  int x[G], c[G];
  float acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int d = d0 + g * GAM_RS_THREADS;
    x[g] = 0;
    c[g] = tl.ts;
    if (d < tl.cnt) {
      if (SINGLE) {
        x[g] = d * tl.O;
      } else {
        const int t = d / tl.N, r = d - t * tl.N;
        x[g] = reinterpret_cast<const int*>(gam_rs_smem)[tl.fs + r] + t * tl.O;
        c[g] = tl.ts + r * tl.pitch;
      }
    }
  }
  if (SINGLE) {
    const float c0 = tl.coeff[0];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = c0 * gam_rs_smem[x[g]];
#pragma unroll 4
    for (int k = 1; k < tl.K; ++k) {
      const float ck = tl.coeff[k];
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = fmaf(ck, gam_rs_smem[x[g] + k], acc[g]);
    }
  } else {
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = gam_rs_smem[c[g]] * gam_rs_smem[x[g]];
#pragma unroll 2
    for (int k = 1; k < tl.K; ++k) {
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = fmaf(gam_rs_smem[c[g] + k], gam_rs_smem[x[g] + k], acc[g]);
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int d = d0 + g * GAM_RS_THREADS;
    if (d < tl.cnt_all) tl.out[d] = d < tl.cnt ? acc[g] : 0.0f;
  }
}

// grid (tiles of L_out, B).  smem: xs [span] | ts [rows, pitch] | fs [rows] (SINGLE: xs only).
template <int FMT, bool SINGLE>
__global__ __launch_bounds__(GAM_RS_THREADS) void gam_resample_kernel(const unsigned char* __restrict__ src, int channels, int channel,
                                                                      const int64_t* __restrict__ len_in, int64_t frames, int64_t row_bytes,
                                                                      int O, int N, int K, int tile, int rows, int pitch, int span,
                                                                      const float* __restrict__ coeff, const int32_t* __restrict__ first,
                                                                      float* __restrict__ dst, int64_t L_out, int64_t* __restrict__ len_out) {
  extern __shared__ float gam_rs_smem[];
  float* xs = gam_rs_smem;
  float* ts = xs + span;
  int* fs = reinterpret_cast<int*>(ts + rows * pitch);
  const int b = blockIdx.y, tid = threadIdx.x;
  int64_t n_in = frames;
  if (len_in != nullptr) { n_in = len_in[b]; n_in = n_in < 0 ? 0 : (n_in > frames ? frames : n_in); }
  int64_t n_out = ((int64_t)N * n_in + O - 1) / O;
  n_out = n_out > L_out ? L_out : n_out;
  if (blockIdx.x == 0 && tid == 0 && len_out != nullptr) len_out[b] = n_out;
  const int64_t j0 = (int64_t)blockIdx.x * tile;
  float* out = dst + (int64_t)b * L_out;
  const int cnt_all = (int)(L_out - j0 < tile ? L_out - j0 : tile);      // outputs this workgroup writes
  if (j0 >= n_out) {                                                     // behind the row's end: the zero padding of the batch
    for (int d = tid; d < cnt_all; d += GAM_RS_THREADS) out[j0 + d] = 0.0f;
    return;
  }
  const int cnt = (int)(n_out - j0 < tile ? n_out - j0 : tile);          // ... of which these are filter outputs
  const int64_t q0 = j0 / N;
  const int p0 = (int)(j0 - q0 * N);
  const int64_t m_lo = first[p0] + q0 * O;                               // base(j0): base is monotone, the tile's span starts here
  // x offset, relative to m_lo, of the tile's output d: base(j0 + d) - m_lo, for d < R = min(cnt, N); output d + t N reads t O further on
  const int R = cnt < N ? cnt : N;
  if (!SINGLE) {
    for (int r = tid; r < R; r += GAM_RS_THREADS) {
      int p = p0 + r, wrap = 0;
      if (p >= N) { p -= N; wrap = 1; }
      fs[r] = (int)(first[p] + (q0 + wrap) * O - m_lo);
      for (int k = 0; k < K; ++k) ts[r * pitch + k] = coeff[(int64_t)p * K + k];
    }
  }
  // the span: base(j0 + cnt - 1) + K - m_lo inputs, converted and downmixed; frames outside [0, n_in) are zeros whatever the row holds there
  int n_span;
  {
    const int64_t jl = j0 + cnt - 1, ql = jl / N;
    n_span = (int)(first[(int)(jl - ql * N)] + ql * O + K - m_lo);
    n_span = n_span > span ? span : n_span;                              // (never: the host sized the tile for it)
  }
  const unsigned char* row = src + (int64_t)b * row_bytes;
  const float inv_c = 1.0f / (float)channels;
  if (channel >= 0 || channels == 1) gam_rs_stage<FMT, 1>(xs, row, m_lo, n_span, n_in, channels, channel < 0 ? 0 : channel, inv_c);
  else if (channels == 2) gam_rs_stage<FMT, 2>(xs, row, m_lo, n_span, n_in, 2, 0, inv_c);
  else gam_rs_stage<FMT, 0>(xs, row, m_lo, n_span, n_in, channels, 0, inv_c);
  __syncthreads();
  // outputs d = tid + 256 i, in groups of 4 / 2 / 1 (the same for every thread of the workgroup) so that each tap's LDS reads are in flight together
  const int per = (cnt_all + GAM_RS_THREADS - 1) / GAM_RS_THREADS;
  const GamRsTile tl = {coeff, out + j0, span, span + rows * pitch, O, N, K, pitch, cnt, cnt_all};
  int i = 0;
  for (; i + 4 <= per; i += 4) gam_rs_outputs<4, SINGLE>(tl, tid + i * GAM_RS_THREADS);
  if (i + 2 <= per) { gam_rs_outputs<2, SINGLE>(tl, tid + i * GAM_RS_THREADS); i += 2; }
  if (i < per) gam_rs_outputs<1, SINGLE>(tl, tid + i * GAM_RS_THREADS);
}

template <int FMT>
static inline hipError_t gam_rs_launch(const GamRsPlan& p, const void* src, int channels, int channel, const int64_t* len_in, int B, int64_t frames,
                                       int bytes_per_sample, const float* coeff, const int32_t* first, float* dst, int64_t L_out, int64_t* len_out,
                                       hipStream_t s) {
  const dim3 grid((unsigned)((L_out + p.tile - 1) / p.tile), (unsigned)B);
  const int64_t row_bytes = frames * channels * bytes_per_sample;
  const unsigned char* sp = static_cast<const unsigned char*>(src);
  if (p.form == GAM_RS_FORM_SINGLE) {
    gam_resample_kernel<FMT, true><<<grid, GAM_RS_THREADS, sizeof(float) * p.span, s>>>(
        sp, channels, channel, len_in, frames, row_bytes, (int)p.O, (int)p.N, p.K, p.tile, 0, p.pitch, p.span, coeff, first, dst, L_out, len_out);
  } else {
    gam_resample_kernel<FMT, false><<<grid, GAM_RS_THREADS, sizeof(float) * (p.span + p.rows * (p.pitch + 1)), s>>>(
        sp, channels, channel, len_in, frames, row_bytes, (int)p.O, (int)p.N, p.K, p.tile, p.rows, p.pitch, p.span, coeff, first, dst, L_out, len_out);
  }
  return hipGetLastError();
}

// 0 = ok, -1 = bad argument, -2 = rate pair refused by the plan, -3 = launch failed
static inline int gam_rs_run(const void* src, int fmt, int channels, int channel, const int64_t* len_in, int B, int64_t frames, int rate_in,
                             int rate_out, const float* coeff, const int32_t* first, float* dst, int64_t L_out, int64_t* len_out, hipStream_t s) {
  if (fmt < 0 || fmt >= GAM_RS_NFMT || channels < 1 || channels > 65535 || channel < -1 || channel >= channels) return -1;
  if (B < 0 || B > 65535 || frames < 0 || L_out < 0 || !coeff || !first) return -1;
  GamRsPlan p;
  const int rc = gam_rs_plan(rate_in, rate_out, &p);
  if (rc != 0) return rc == -1 ? -1 : -2;
  if (B == 0 || L_out == 0) return 0;
  if (!dst || (!src && frames > 0)) return -1;
  if ((L_out + p.tile - 1) / p.tile > 0x7fffffffLL) return -1;
  hipError_t e;
  switch (fmt) {
    case GAM_RS_U8: e = gam_rs_launch<GAM_RS_U8>(p, src, channels, channel, len_in, B, frames, 1, coeff, first, dst, L_out, len_out, s); break;
    case GAM_RS_I16: e = gam_rs_launch<GAM_RS_I16>(p, src, channels, channel, len_in, B, frames, 2, coeff, first, dst, L_out, len_out, s); break;
    case GAM_RS_I24: e = gam_rs_launch<GAM_RS_I24>(p, src, channels, channel, len_in, B, frames, 3, coeff, first, dst, L_out, len_out, s); break;
    case GAM_RS_I32: e = gam_rs_launch<GAM_RS_I32>(p, src, channels, channel, len_in, B, frames, 4, coeff, first, dst, L_out, len_out, s); break;
    case GAM_RS_F32: e = gam_rs_launch<GAM_RS_F32>(p, src, channels, channel, len_in, B, frames, 4, coeff, first, dst, L_out, len_out, s); break;
    case GAM_RS_MULAW: e = gam_rs_launch<GAM_RS_MULAW>(p, src, channels, channel, len_in, B, frames, 1, coeff, first, dst, L_out, len_out, s); break;
    default: e = gam_rs_launch<GAM_RS_ALAW>(p, src, channels, channel, len_in, B, frames, 1, coeff, first, dst, L_out, len_out, s); break;
  }
  return e == hipSuccess ? 0 : -3;
}
