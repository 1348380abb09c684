// gam_gemm_sp.h -- the split-fp16 GEMM: (64 MT) x (64 NW) block tiles fed entirely by
// LDS-DMA (global_load_lds_dwordx4), two or three LDS stages, one barrier per k-tile.
//
// Three-term split ("f16x3") on the fp16 matrix cores (v_mfma_f32_16x16x32_f16, 16x the
// rate of the fp32 MFMA), fp32 accumulate:
//
//   a = a_hi + a_lo,  w * 2^s = w_hi + w_lo      (hi = fp16(x), lo = fp16(x - hi))
//   a.w ~= (a_hi.w_hi + a_hi.w_lo + a_lo.w_hi) * 2^-s
//
// fp16 carries 11 significant bits, so hi+lo keeps 22 of fp32's 24 and the dropped a_lo.w_lo
// term is ~2^-22 relative: on the full 16-layer encoder the split path is as close to an fp64
// evaluation as plain fp32 is.  The power-of-two pre-scale of each weight
// matrix (exact, undone in the epilogue, gam_api.hip make_split) keeps w_lo clear of the fp16
// subnormal range.  Both operands arrive already split, in the "sp32" layout that the producing
// kernels write instead of fp32:
//
//   element (row, k)  ->  halfs  row*2K + (k/32)*64 + (k%32)        hi = fp16(x)
//                                row*2K + (k/32)*64 + 32 + (k%32)   lo = fp16(x - hi)
//
// i.e. the 4 bytes an fp32 element would occupy hold its (hi, lo) pair, regrouped so that one
// row's share of a 32-deep k-tile is ONE 128-byte line [hi x32 | lo x32].  A k-tile of a block is
// then (BM + 256) full lines; a wave-wide global_load_lds_dwordx4 moves 8 of them (1 KiB) straight
// into LDS -- no staging registers, no ds_write pass, no conversion in the GEMM.  (A 128x128
// register-staged kernel measured TD/TCP-bound on exactly that traffic: profiles/r01_f16x3_*.)
//
// LDS image: rows of 128 B (8 slots of 16 B), slot' = slot ^ key(row), key bits (r1, r2 ^ r4, r3) of the row's index in its
// operand's block tile (gam_sp_key).  LDS-DMA writes lane-linear, so the XOR is applied to the per-lane SOURCE address; fragment
// reads apply the same XOR.  Conflicts, re-derived for the rows the 16x16x32 fragments read: lane l reads operand row i = l & 15 at
// logical slot 4 plane + (l >> 4), and a ds_read_b128 is served in four 16-lane groups, lanes {0-3, 12-15, 20-27} etc. -- i in
// {0-3, 12-15} at slot s and i in {4-11} at slot s ^ 1.  A group is conflict-free when (row & 1, slot') differ over its 16 lanes.
//   activation block: rows 16 b + i, key = (i1, i2 ^ b0, i3); the s ^ 1 lanes are those with i2 ^ i3 = 1, so the low slot bits are
//     (i1 ^ i2 ^ i3, i2 ^ b0, i3) with row parity i0: a bijection of i.
//   W block 2 p + t: rows 32 p + 8 (i >> 2) + 4 t + (i & 3) (the row order that gives a lane 8 consecutive C columns, see the
//     epilogue), i.e. r0 = i0, r1 = i1, r2 = t, r3 = i2, r4 = i3: key = (i1, t ^ i3, i2) -> (i1 ^ i2 ^ i3, t ^ i3, i2): a bijection.
//     (The r4 term is what this row order needs: with the plain (row >> 1) & 7 rows i and i + 8 of the block collide.)
// Conflict-free without padding for both operands.
//
// 2 (M) x NW (N) waves; a wave owns (32 MT) x 64 outputs = 2 MT x 4 blocks of 16 x 16, 3 MFMAs per block per
// 32-deep k-tile.  At NW = 4 (256-wide tiles, one workgroup per CU) the bytes moved per FLOP are half
// those of a 128 x 128 tile; the k-tile after next lands while the current one is multiplied.
// Why this MFMA shape: same cycles per FLOP as 32x32x16, same LDS bytes, but under the power cap the chip holds a higher clock
// on it (measurements: profiles/mfma16_gemm_ab.md).
// MT in {2,3,4} and NW in {2,4} are picked per launch (gam_gemm_sp_plan) to minimise the tail of the
// last round of tiles.
#pragma once
#include "gam_gemm.h"
#include <type_traits>
#if defined(GAM_SP_INSTRUMENT) && GAM_SP_INSTRUMENT
#include <algorithm>
#include <vector>
#endif

// -DGAM_SP_INSTRUMENT=1 is the one instrumented build: the per-workgroup timeline, turned on at run time by GAM_SP_TLOG=1 -- wall clock
// (100 MHz) at entry / operands of the first two k-tiles landed / main loop done / epilogue done, shader clock around the loop -- into
// g.tlog[tile * 8 ..]; the launcher prints the distribution (tools/gemm_sp_test.py; profiles/r03_gemm_timeline.txt).  It measures and
// changes nothing the kernel computes; production builds carry none of it.
#ifndef GAM_SP_INSTRUMENT
#define GAM_SP_INSTRUMENT 0
#endif
#if GAM_SP_INSTRUMENT
#define GAM_SP_TL(i)                                                                  \
  if (g.tlog != nullptr && threadIdx.x == 0) {                                        \
    g.tlog[(size_t)lid * 8 + (i)] = wall_clock64();                                   \
    if ((i) == 1 || (i) == 2) g.tlog[(size_t)lid * 8 + 4 + (i)] = clock64();          \
    if ((i) == 0) g.tlog[(size_t)lid * 8 + 7] = blockIdx.x;                            \
  }
#else
#define GAM_SP_TL(i)
#endif

template <int MT, int NW, int NS = 2>
struct GamGemmSpCfg {
  static constexpr int BM = 64 * MT;
  static constexpr int BN = 64 * NW;
  static constexpr int NWAVES = 2 * NW;                 // 2 (M) x NW (N) waves
  static constexpr int NT = 64 * NWAVES;
  static constexpr int A_BYTES = BM * 128;
  static constexpr int W_BYTES = BN * 128;
  static constexpr int STAGE = A_BYTES + W_BYTES;
  static constexpr int SMEM = NS * STAGE;      // NS LDS stages: the k-tiles kt .. kt + NS - 1 are resident / in flight
  static constexpr int NAI = BM / 8 / NWAVES;   // A DMA pieces per wave per k-tile (8 rows x 128 B each)
  static constexpr int NWI = BN / 8 / NWAVES;   // W DMA pieces per wave per k-tile
};

// XOR key of the LDS image: slot' = slot ^ gam_sp_key(row), row = the row's index in its operand's block tile.  Bits (r1, r2 ^ r4, r3).
__device__ __forceinline__ int gam_sp_key(int row) { return ((row >> 1) & 7) ^ ((row >> 3) & 2); }

// NS = LDS stages.  2: the k-tile after next lands while the current one is multiplied -- enough for the 8-wave tiles, whose
// k-tile takes 1.4-1.8 us of MFMA work.  3 (r04, the 4-wave tiles of small grids): a 128 x 128 k-tile is 0.3 us of MFMA work but
// its 32 KB take ~0.8 us from issue to landed, and with two stages exactly ONE k-tile of fetch is in flight, so the loop ran at
// the fetch latency (per-workgroup timeline, profiles/r04_gemm_timeline_m2008.txt: 0.78 us per k-tile at M = 2008 whatever the
// shape).  With three stages TWO k-tiles are in flight: the in-loop wait is a counted vmcnt (the newest tile's pieces may still
// be outstanding) in front of a bare s_barrier -- __syncthreads() would drain the queue (cdna_hip_programming.md, glds rule).
// H16 (r04, the opt-in GAM_GEMM_F16 speed mode): ONE fp16 MFMA per product -- the arithmetic contract of the reference's own GPU
// default (fp16 autocast, /root/reference/gigaam/model.py:34-37), fp32 accumulation.  Both operands are then PLAIN fp16 rows
// (the producing kernels store format 2 of gam_store4: the fp16 of each value, row-major), and the kernel is told HALF the
// reduction length: a row's 128-byte share of a "k-tile" holds 64 consecutive fp16 values instead of 32 (hi, lo) pairs, so the
// DMA, the LDS image, the swizzle and the fragment reads are exactly those of the three-term kernel -- what used to be the lo
// half of the line is simply the next 32 k-values -- and the MFMA stream multiplies (first half x first half) + (second half x
// second half): two K = 32 MFMAs per 16 x 16 x 64 block instead of three per 16 x 16 x 32.  Per unit of K: a third of the matrix
// work, half the operand bytes.  (A first version kept the sp32 operands and fetched only the hi half of every line: a 64-byte
// piece of each 128-byte line costs the memory path the whole line, and the kernel ran at half the delivery rate --
// profiles/r04_fastmode.txt.)
//
// EPI = the epilogue class: which of the epilogue's options this instantiation carries, as compile-time bits.  The options are run-time
// fields of GamGemmArgs; tested per element or per 16-byte piece inside the unrolled row loop they made the FFN-up epilogue 5205
// instructions where its class needs 1562 (profiles/gemm_epilogue_classes.md) -- paid with the matrix pipe idle.  The launcher
// derives the bits from the arguments (gam_sp_epi_bits) and picks the instantiation of the same bits if the encoder's callers can
// produce them (gam_launch_gemm_sp lists them); everything else runs GAM_EPI_GENERIC, which reads every option from GamGemmArgs at
// run time.  One body serves both: an option is `GEN ? run-time field : class bit`, a constant wherever the class decides it.  No
// class changes a rounding -- the order on a value stays acc * rsc + bias -> activation -> mask -> * alpha -> + R -> split, and the
// multiply a class drops is by exactly 1.0f.
enum : int {
  GAM_EPI_SP32 = 1,      // C in the sp32 layout (c_split 1)
  GAM_EPI_F16 = 2,       // C as plain fp16 rows (c_split 2)
  GAM_EPI_CFMT = 3,
  GAM_EPI_RESID = 4,     // + R
  GAM_EPI_ALPHA = 8,     // alpha != 1
  GAM_EPI_ROWS = 16,     // row mask and / or row remap (lens != nullptr || remap)
  GAM_EPI_GUARD = 32,    // range guard on C (c_guard with a flag word)
  GAM_EPI_TAIL = 64,     // N % 8 == 4: the last 8-column group of a row has its first half only
  GAM_EPI_PART = 128,    // split-K slice: raw partial sums, no other option applies
  GAM_EPI_GENERIC = 256  // every option read from GamGemmArgs at run time
};

template <int ACT, int EPI, int MT, int NW, int NS = 2, bool H16 = false>
__global__ __launch_bounds__(128 * NW, NW == 2 ? 2 : 1) void gam_gemm_sp_kernel(GamGemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gam_smem_sp[];
  using Cfg = GamGemmSpCfg<MT, NW, NS>;
  constexpr int BM = Cfg::BM, BN = Cfg::BN, NAI = Cfg::NAI, NWI = Cfg::NWI, NWAVES = Cfg::NWAVES;
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef const __attribute__((address_space(1))) void* glb_ptr_t;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / NW, wn = wave % NW;

  const int nbn = (g.N + BN - 1) / BN;
  const int total = gridDim.x;
  const int q8 = total >> 3, r8 = total & 7;
  const int bid = blockIdx.x;
  const int xcd = bid & 7;
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  int tm = lid / nbn, tn = lid % nbn;
  if (g.skip_pad) {
    // An XCD's CONTIGUOUS share of the tiles is a run of utterances: the XCDs of the short ones would finish early and wait for the one that
    // holds the longest (measured: no gain at all).  The tiles are dealt round robin over the XCDs instead.  (Keeping the column tiles of a
    // row tile on one XCD -- they share the A patch -- measured worse: conv2 0.955 of the padded launch against 0.905, r06_packed_rows_ab.txt.)
    tm = bid / nbn;
    tn = bid % nbn;
  }
  const int m0 = tm * BM;
  const int n0 = tn * BN;
  if (g.skip_pad && g.lens != nullptr) {   // (uniform: the whole workgroup leaves before its first DMA and barrier)
    const int mlast = m0 + BM - 1 < g.M ? m0 + BM - 1 : g.M - 1;
    const int b0 = m0 / g.rpb;
    if (b0 == mlast / g.rpb && (m0 - b0 * g.rpb) / g.fdiv >= g.lens[b0]) return;
  }
  GAM_SP_TL(0);

  // ---- DMA sources.  Piece q of an operand = tile rows 8q .. 8q+7; this wave moves pieces
  //      q = wave + NWAVES i.  Lane l -> row 8q + (l>>3), LDS slot' l&7, source slot (l&7) ^ gam_sp_key(row).
  //      Addresses = wave-uniform tile base (SGPR pair) + 32-bit lane offset.
  auto a_row_off = [&](int m) -> size_t {
    m = m < g.M ? m : g.M - 1;
    if (g.a_mode == 0) return (size_t)m * (size_t)g.lda;
    const int fr = m / g.conv_f2, ff = m - fr * g.conv_f2;
    return ((size_t)fr * 2 * g.conv_fp + 2 * ff) * (size_t)g.conv_c;
  };
  const size_t a_tile0 = a_row_off(m0);   // offsets grow with m, so every row offset is >= this one
  const unsigned char* Ab = reinterpret_cast<const unsigned char*>(g.n_switch > 0 && n0 >= g.n_switch ? g.Asp2 : g.Asp) + a_tile0 * 4;
  const unsigned char* Wb = reinterpret_cast<const unsigned char*>(g.Wsp) + (size_t)n0 * (size_t)g.K * 4;
  unsigned a_src[NAI], w_src[NWI];
#pragma unroll
  for (int i = 0; i < NAI; ++i) {
    const int row = 8 * (wave + NWAVES * i) + (lane >> 3);
    const int slot = (lane & 7) ^ gam_sp_key(row);
    a_src[i] = (unsigned)((a_row_off(m0 + row) - a_tile0) * 4) + slot * 16;
  }
#pragma unroll
  for (int i = 0; i < NWI; ++i) {
    const int row = 8 * (wave + NWAVES * i) + (lane >> 3);
    const int slot = (lane & 7) ^ gam_sp_key(row);
    int n = n0 + row;
    n = n < g.N ? n : g.N - 1;
    w_src[i] = (unsigned)(n - n0) * (unsigned)g.K * 4u + slot * 16;
  }

  f32x4 acc[2 * MT][4];   // [16-row block of C][16-column block]: the wave's (32 MT) x 64 outputs
#pragma unroll
  for (int i = 0; i < 2 * MT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

  // split-K (grid.y = g.splitk slices, small grids: a few utterances per GPU): this workgroup contracts k-tiles
  // [kt_first, kt_first + nk) and leaves raw partial sums in g.partial[slice]; gam_splitk_reduce_kernel sums the slices in
  // a fixed order (bit-reproducible) and applies the epilogue.  One slice = the whole K = the plain kernel.
  const int nslice = g.splitk > 1 ? g.splitk : 1;
  const int nk = g.K / 32 / nslice;
  const int kt_first = (nslice > 1 ? (int)blockIdx.y : 0) * nk, kt_end = kt_first + nk;
  // next k-tile to fetch, tracked incrementally (no divisions in the loop); it stops at the slice's last tile
  int d_kt = kt_first, d_c0 = 0, d_kw = 0, d_kh = 0;
  if (g.a_mode != 0) {   // taps innermost: k-tile = 9 * (32-channel block) + 3 kh + kw
    const int cb = kt_first / 9, t9 = kt_first - cb * 9;
    d_c0 = 32 * cb; d_kh = t9 / 3; d_kw = t9 - d_kh * 3;
  }
  auto dma_ka = [&]() -> size_t {   // byte offset of tile d_kt along an A row
    if (g.a_mode == 0) return (size_t)d_kt * 128;
    return (((size_t)d_kh * g.conv_fp + d_kw) * (size_t)g.conv_c + d_c0) * 4;
  };
  // conv mode walks the taps INNERMOST: the nine k-tiles of a 32-channel block re-read the same (2 rows + 1) x (2 cols
  // + 1) pixel patch of the tile, shifted -- 139 KB per workgroup, L2-resident -- instead of streaming the whole
  // 768-channel image once per tap (the weight's sp32 copy is laid out in the same k-tile order, make_split)
  auto dma_advance = [&]() {
    if (d_kt + 1 >= kt_end) return;
    ++d_kt;
    if (g.a_mode == 0) return;
    if (++d_kw == 3) {
      d_kw = 0;
      if (++d_kh == 3) { d_kh = 0; d_c0 += 32; }
    }
  };
  auto issue = [&](int stage) {
    unsigned char* sb = gam_smem_sp + stage * Cfg::STAGE + wave * 1024;
    const unsigned char* ab = Ab + dma_ka();
    const unsigned char* wb = Wb + (size_t)d_kt * 128;
#pragma unroll
    for (int i = 0; i < NAI; ++i)
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(ab + a_src[i]), (lds_ptr_t)(sb + i * (NWAVES * 1024)), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < NWI; ++i)
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(wb + w_src[i]), (lds_ptr_t)(sb + Cfg::A_BYTES + i * (NWAVES * 1024)), 16, 0, 0);
    dma_advance();
  };

  // ---- fragment addressing (v_mfma_f32_16x16x32_f16: lane l supplies operand row l & 15, halves k = 8 (l >> 4) .. + 7):
  //      one ds_read_b128 = logical slot 4 plane + (l >> 4) of a row.  Activation block i = tile rows a_base + 16 i + (l & 15).
  //      W block T = 2 p + t = tile rows w_base + 32 p + 8 ((l & 15) >> 2) + 4 t + (l & 3): lane group l >> 4 = q then holds the
  //      C columns 32 p + 8 q + 4 t .. + 3 of block T, i.e. EIGHT consecutive columns over the block pair (2 p, 2 p + 1).
  const int fi = lane & 15, fg = lane >> 4;
  const int wr = 8 * (fi >> 2) + (fi & 3);
  int o_a[2][2], o_w[2][2];   // [plane][row bit 4 of the block (i & 1) | t]
#pragma unroll
  for (int pl = 0; pl < 2; ++pl)
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      o_a[pl][x] = fi * 128 + (((4 * pl + fg) ^ gam_sp_key(fi + 16 * x)) << 4);
      o_w[pl][x] = (wr + 4 * x) * 128 + (((4 * pl + fg) ^ gam_sp_key(wr + 4 * x)) << 4);
    }
  const int a_base = wm * (BM / 2) * 128;   // (BM / 2 = 32 MT rows: a multiple of 32, so row bit 4 of block i is i & 1)
  const int w_base = Cfg::A_BYTES + wn * 64 * 128;

  // ONE fragment set (a whole k-tile of 16x16x32 operands is 16 MT + 32 registers: two do not fit beside the 32 MT accumulators).
  // The k-tile's MFMAs run as four quadrants of the wave tile -- activation halves M0 / M1 (MT blocks each) x W halves N0 / N1
  // (two blocks each) -- and an operand half is refilled for the next k-tile as soon as its last MFMA has issued:
  //   quadrant 1 (M0,N0): reads N1, then M1 (both of THIS tile: their registers were busy to the end of the last one)
  //   quadrant 2 (M0,N1): MFMAs only
  //   vmcnt + lgkmcnt(0) + barrier     -- tile kt+1 landed everywhere, stage of tile kt has no reader left
  //   quadrant 3 (M1,N0): reads M0 of tile kt+1, then DMA pieces of tile kt+NS -> stage of tile kt
  //   quadrant 4 (M1,N1): reads N0 of tile kt+1, then the rest of the DMA pieces
  // The last quadrant shares no operand half with the first, so one loop body serves every k-tile.  Per accumulator the order
  // is the same everywhere: k-tiles ascending, terms hi.hi, lo_w.hi_a, hi_w.lo_a.
  // Everything that is not an MFMA is issued one or two items at a time BETWEEN MFMAs: an LDS-DMA piece
  // costs the issuing wave ~60+ cycles, and with the whole refill issued in one block after the barrier
  // both waves of a SIMD sat in it together and the matrix pipe idled ~600 of every 3500 cycles
  // (clock64 counters around the halves of the k-tile, profiles/r01_gemm_sp_clock_random_vs_zero.txt).
  gam_half8 fah[2 * MT], fal[2 * MT], fwh[4], fwl[4];
  constexpr int NTERM = H16 ? 2 : 3;
  constexpr int QM = 2 * NTERM * MT;  // MFMAs per quadrant: terms x MT x 2 blocks
  constexpr int NG = NAI + NWI;       // DMA pieces per wave per k-tile
  // One item per MFMA slot: a 16x16x32 MFMA holds the vector issue for 8 of its 16 cycles, which hides one ds_read_b128, not two
  // (with one wave per SIMD -- the 4-wave tiles of small grids -- whatever does not fit is exposed).  Quadrant 3 carries its 2 MT
  // reads, then DMA pieces; quadrant 4 its 4 reads, then the remaining pieces.
  constexpr int G3 = QM - 2 * MT;     // DMA pieces carried by quadrant 3
  static_assert(4 + 2 * MT <= QM && G3 + QM - 4 >= NG, "quadrant too short for its reads + DMA pieces");
#define GAM_SPLD(P) (*reinterpret_cast<const gam_half8*>(P))
  // (plain ifs on unrolled loop counters, not nested generic lambdas: those push the fragment arrays to scratch)
  // read item Q of W half NH: blocks 2 NH, 2 NH + 1, hi plane first
#define GAM_SP_RDW(NH, Q, ST)                                                                     \
  {                                                                                               \
    const int q_ = (Q);                                                                           \
    if (q_ < 2) fwh[2 * (NH) + (q_ & 1)] = GAM_SPLD((ST) + w_base + (NH) * 4096 + o_w[0][q_ & 1]);  \
    else fwl[2 * (NH) + (q_ & 1)] = GAM_SPLD((ST) + w_base + (NH) * 4096 + o_w[1][q_ & 1]);         \
  }
  // read item Q of activation half MH: blocks MH MT .. MH MT + MT - 1, hi plane first
#define GAM_SP_RDA(MH, Q, ST)                                                                     \
  {                                                                                               \
    const int q_ = (Q), i_ = (MH) * MT + q_ % MT;                                                 \
    if (q_ < MT) fah[i_] = GAM_SPLD((ST) + a_base + i_ * 2048 + o_a[0][i_ & 1]);                  \
    else fal[i_] = GAM_SPLD((ST) + a_base + i_ * 2048 + o_a[1][i_ & 1]);                          \
  }
#define GAM_SP_MFMA(MH, NH, T)                                                                    \
  {                                                                                               \
    const int term_ = (T) / (2 * MT), i_ = (MH) * MT + ((T) % (2 * MT)) / 2, j_ = 2 * (NH) + ((T) & 1); \
    /* three terms: hi.hi, lo_w.hi_a, hi_w.lo_a;  H16: first-half x first-half, second-half x second-half */ \
    acc[i_][j_] = __builtin_amdgcn_mfma_f32_16x16x32_f16(term_ == 1 ? fwl[j_] : fwh[j_],          \
                                                         (H16 ? term_ == 1 : term_ == 2) ? fal[i_] : fah[i_], acc[i_][j_], 0, 0, 0); \
  }
  // first half of a k-tile: quadrants (M0, N0) and (M0, N1); reads N1 and M1 of this tile (stage st)
  auto half0 = [&](const unsigned char* st) {
#pragma unroll
    for (int t = 0; t < QM; ++t) {
      GAM_SP_MFMA(0, 0, t);
      if (t < 4) GAM_SP_RDW(1, t, st)
      else if (t < 4 + 2 * MT) GAM_SP_RDA(1, t - 4, st)
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int t = 0; t < QM; ++t) {
      GAM_SP_MFMA(0, 1, t);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // second half: quadrants (M1, N0) and (M1, N1); reads M0 and N0 of the next tile (stage sn); DMA -> stage istage
  auto half1 = [&](const unsigned char* sn, int istage) {
    const unsigned char* ab = Ab + dma_ka();
    const unsigned char* wb = Wb + (size_t)d_kt * 128;
    unsigned char* sb = gam_smem_sp + istage * Cfg::STAGE + wave * 1024;
    dma_advance();
#pragma unroll
    for (int u = 0; u < 2 * QM; ++u) {
      if (u < QM) {
        GAM_SP_MFMA(1, 0, u);
        if (u < 2 * MT) GAM_SP_RDA(0, u, sn)
      } else {
        GAM_SP_MFMA(1, 1, u - QM);
        if (u - QM < 4) GAM_SP_RDW(0, u - QM, sn)
      }
      const int gi = u < QM ? u - 2 * MT : (u - QM < 4 ? -1 : G3 + u - QM - 4);
      if (gi >= 0 && gi < NG) {
        if (gi < NAI)
          __builtin_amdgcn_global_load_lds((glb_ptr_t)(ab + a_src[gi % NAI]), (lds_ptr_t)(sb + gi * (NWAVES * 1024)), 16, 0, 0);
        else
          __builtin_amdgcn_global_load_lds((glb_ptr_t)(wb + w_src[(gi - NAI + NWI) % NWI]),
                                           (lds_ptr_t)(sb + Cfg::A_BYTES + (gi - NAI) * (NWAVES * 1024)), 16, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // in-loop wait: everything but the newest (NS - 2) k-tiles' DMA pieces of this wave has landed (vmcnt counts in issue order)
  constexpr int VMW = (NS - 2) * NG;
  static_assert(VMW < 64, "vmcnt field");
#pragma unroll
  for (int st_ = 0; st_ < NS; ++st_) issue(st_);   // (fewer k-tiles than stages: the last one is fetched again, unused)
  if constexpr (NS == 2) {
    __builtin_amdgcn_s_waitcnt(0x0070);
    __syncthreads();   // both tiles have landed for every wave
  } else {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(VMW) : "memory");   // tiles 0 and 1 have landed for every wave
  }
  GAM_SP_TL(1);
  // a k-tile starts on (M0, N0)
#pragma unroll
  for (int q = 0; q < 2 * MT; ++q) GAM_SP_RDA(0, q, gam_smem_sp);
#pragma unroll
  for (int q = 0; q < 4; ++q) GAM_SP_RDW(0, q, gam_smem_sp);
  int s_cur = 0;       // LDS stage of k-tile kt
  for (int kt = 0; kt < nk; ++kt) {
    const int s_nxt = s_cur + 1 == NS ? 0 : s_cur + 1;
    const unsigned char* st = gam_smem_sp + s_cur * Cfg::STAGE;
    const unsigned char* sn = gam_smem_sp + s_nxt * Cfg::STAGE;
    half0(st);
    // vmcnt by hand: this wave's DMA pieces of tile kt+1 have landed (hipcc does not order an LDS-DMA against the
    // ds_reads behind a later barrier); lgkmcnt(0): this wave's last reads of tile kt are in registers
    if constexpr (NS == 2) {
      __builtin_amdgcn_s_waitcnt(0x0070);
      __syncthreads();
    } else {
      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(VMW) : "memory");
    }
    // Unconditional (one copy of the MFMA stream; a second, DMA-less copy behind a branch made hipcc
    // double-buffer the accumulators): past the end the reads fetch stale LDS that is never used
    // and the DMA re-fetches the last k-tile into a stage nobody reads again (drained before the epilogue).
    // The refill goes to the stage of tile kt: every wave has read its last fragments before the barrier above.
    half1(sn, s_cur);
    s_cur = s_nxt;
  }
#undef GAM_SPLD
#undef GAM_SP_RDW
#undef GAM_SP_RDA
#undef GAM_SP_MFMA
  // every LDS-DMA piece of this wave has landed (a workgroup must not retire with DMA writes in flight: its LDS
  // could already belong to the next one); no barrier -- the epilogue below touches no shared memory
  __builtin_amdgcn_s_waitcnt(0x0070);
  GAM_SP_TL(2);

  const int mw = m0 + wm * (BM / 2), nw = n0 + wn * 64;

  // ---- epilogue, straight from the accumulators.  The MFMAs run with the operands SWAPPED (W fragment as the A
  //      operand, activation fragment as B), i.e. they accumulate C^T blocks: lane l then owns ONE row of C per block row
  //      (m = 16 i + (l & 15)) and, in block T = 2 p + t, the FOUR CONSECUTIVE columns 32 p + 8 (l >> 4) + 4 t + r (r = register;
  //      the W rows were dealt to the A-operand rows that way, see the fragment addressing).  Bias / residual / C therefore move
  //      as 16-byte vectors with no transpose: the former per-wave LDS round trip (96 ds_write_b32 + 24 ds_read_b128 per wave, 8
  //      waves on one LDS) cost 5.0 of the 7.3 us a 192 x 256 tile spent here (profiles/r03_gemm_timeline.txt).
  // (r04, tried and dropped: requesting the bias pieces and the row scales of the 4-wave tiles in front of the first k-tile, so
  //  that the epilogue of a small-grid launch does not start with an L2 round trip -- 32 + MT more live registers, same-box A/B
  //  6.22-6.24 vs 6.24-6.25 ms at 4 x 20 s, 2.85 vs 2.89 ms for one clip: nothing; profiles/r04_ab_experiments.txt)
  // r04: EIGHT consecutive columns per lane -- the blocks 2 p and 2 p + 1 hold the two halves of the lane's 8-column group: bias /
  // residual / C move as pairs of adjacent 16-byte pieces (the four lane groups complete a row's 128-byte line per instruction pair),
  // and an sp32 / fp16 result as ONE 16-byte store per plane instead of two 8-byte ones (the store path, not the arithmetic, is what
  // an epilogue costs: profiles/r03_gemm_timeline.txt).  On the 32x32x16 shape this took a v_permlane32_swap per register; here it is
  // address arithmetic alone.
  // The options are compile-time per epilogue class (EPI, above); the range guard keeps a running maximum per lane and tests it
  // once; a lane's column offsets are computed once and a row adds its pitch once (profiles/gemm_epilogue_classes.md).
  constexpr bool GEN = (EPI & GAM_EPI_GENERIC) != 0;
  const bool part = GEN ? g.partial != nullptr : (EPI & GAM_EPI_PART) != 0;
  const int cfmt = GEN ? g.c_split : (EPI & GAM_EPI_CFMT);
  const bool resid = !part && (GEN ? g.R != nullptr : (EPI & GAM_EPI_RESID) != 0);
  const bool scaled = GEN || (EPI & GAM_EPI_ALPHA) != 0;          // (the generic class multiplies by alpha whatever it is: 1.0f is exact)
  const bool need_bt = !part && (GEN ? (g.lens != nullptr || g.remap) : (EPI & GAM_EPI_ROWS) != 0);
  const bool guard = GEN ? (g.c_guard && g.range_flag != nullptr) : (EPI & GAM_EPI_GUARD) != 0;
  const bool tail = GEN ? (g.N & 4) != 0 : (EPI & GAM_EPI_TAIL) != 0;
  const int lrow = lane & 15, lq8 = (lane >> 4) * 8;
  const float accscale = g.wscale_inv;
  // Column data, once per lane.  Piece (p, hf): columns ecol0 + 32 p + 4 hf .. + 3  =  accumulator block 2 p + hf.  Group p = 1 lies 32
  // columns behind group 0 in every format: 128 bytes in fp32 and in sp32 (the next [hi x32 | lo x32] line), 64 in plain fp16.
  const int ecol0 = nw + lq8;                                    // first of this lane's eight columns of group 0
  bool c_ok[2], c_both[2];
#pragma unroll
  for (int pp = 0; pp < 2; ++pp) {
    c_ok[pp] = ecol0 + 32 * pp < g.N;
    c_both[pp] = !tail || ecol0 + 32 * pp + 4 < g.N;             // (N % 8 == 4: the last group has its first half only)
  }
  f32x4 bv[2][2];
#pragma unroll
  for (int pp = 0; pp < 2; ++pp)
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int col = ecol0 + 32 * pp + 4 * hf;
      bv[pp][hf] = (g.bias != nullptr && col < g.N) ? *reinterpret_cast<const f32x4*>(g.bias + col) : (f32x4){0.f, 0.f, 0.f, 0.f};   // N % 4 == 0
    }
  // byte offset of the lane's group 0 inside a row of C, the row pitch and the step to group 1
  const long c_col = cfmt == 1 ? 2L * ((ecol0 >> 5) * 64 + (ecol0 & 31)) : (cfmt == 2 ? 2L * ecol0 : 4L * ecol0);
  const long c_pitch = cfmt == 2 ? 2 * g.ldc : 4 * g.ldc;
  const int c_step = cfmt == 2 ? 64 : 128;
  unsigned char* const c_base = reinterpret_cast<unsigned char*>(g.C) + c_col;
  // Row data of all 2 MT rows first -- validity, mask, output row, per-row factor -- so that the a_rs / lens loads of every row
  // are in flight together: inside the row loop each would sit behind the previous row's stores (C may alias anything), one
  // exposed L2 round trip per row, and the 16-row blocks make twice as many rows per lane as the 32-row blocks did.
  // (utterance, frame) of a row: ONE division per lane -- a lane's rows are 16 apart, so the next row's pair follows by a
  // conditional subtraction (utterances of fewer than 16 rows divide again); the mask test tt / fdiv >= len is tt >= len fdiv.
  // A split-K slice needs neither (it stores raw sums of every row below M), nor does a class without mask and remap: there the
  // output row is the row and nothing but the per-row factor is kept.  Measured on the small grids, where the epilogue
  // is a visible share of a launch: profiles/mfma16_gemm_ab.md, section 4.
  bool r_ok[2 * MT], r_masked[2 * MT];
  long r_orow[2 * MT];
  float r_rsc[2 * MT];
  int bb = 0, tt = 0;
  if (need_bt) { bb = (mw + lrow) / g.rpb; tt = (mw + lrow) - bb * g.rpb; }
#pragma unroll
  for (int i = 0; i < 2 * MT; ++i) {
    const int row = mw + 16 * i + lrow;
    bool ok = row < g.M, masked = false;
    long orow = row;
    if (need_bt) {
      if (i > 0) {
        tt += 16;
        if (g.rpb < 16) { bb = row / g.rpb; tt = row - bb * g.rpb; }
        else if (tt >= g.rpb) { tt -= g.rpb; ++bb; }
      }
      if (ok) {
        if (g.lens != nullptr) masked = tt >= g.lens[bb] * g.fdiv;
        if (g.remap) {
          if (tt >= g.rows_valid) ok = false;
          orow = (long)bb * g.out_rpb + tt + g.out_shift;
        }
      }
    }
    // per-row factor (weight scale x the A operand's row scale)
    r_rsc[i] = accscale * ((ok && g.a_rs != nullptr) ? g.a_rs[row] : 1.0f);
    r_ok[i] = ok; r_masked[i] = masked; r_orow[i] = orow;
  }
  if (part) {   // split-K slice: scaled raw sums; bias / activation / residual belong to the reduce pass
#pragma unroll
    for (int i = 0; i < 2 * MT; ++i) {
      if (!r_ok[i]) continue;
      float* P = g.partial + ((size_t)blockIdx.y * (size_t)g.M + (size_t)(mw + 16 * i + lrow)) * (size_t)g.N + ecol0;
#pragma unroll
      for (int pp = 0; pp < 2; ++pp)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
          if (ecol0 + 32 * pp + 4 * hf < g.N) *reinterpret_cast<f32x4*>(P + 32 * pp + 4 * hf) = acc[i][2 * pp + hf] * r_rsc[i];
    }
  }
  // the four residual pieces of row I -> D; the pieces of row i + 1 are requested BEFORE row i is stored (a lane reads and writes
  // only its own elements, so R == C is safe), which keeps one row of residual in flight behind every row of stores
#define GAM_SP_LDR(I, D)                                                                          \
  {                                                                                               \
    const float* rrow_ = g.R + r_orow[I] * g.ldr + ecol0;                                         \
    _Pragma("unroll") for (int pp = 0; pp < 2; ++pp) _Pragma("unroll") for (int hf = 0; hf < 2; ++hf)  \
      D[pp][hf] = (r_ok[I] && ecol0 + 32 * pp + 4 * hf < g.N) ? *reinterpret_cast<const f32x4*>(rrow_ + 32 * pp + 4 * hf)  \
                                                             : (f32x4){0.f, 0.f, 0.f, 0.f};       \
  }
  f32x4 rv[2][2], rn[2][2];
  float gmax = 0.f;   // range guard: the largest |value| this lane stores (fmaxf drops a NaN, as the per-piece test did; an Inf stays)
  if (resid) GAM_SP_LDR(0, rv);
#pragma unroll
  for (int i = 0; i < 2 * MT; ++i) {
    if (resid && i + 1 < 2 * MT) GAM_SP_LDR(i + 1, rn);
    const bool masked = r_masked[i];
    const float rsc = r_rsc[i];
    if (r_ok[i] && !part) {
      unsigned char* const crow = c_base + r_orow[i] * c_pitch;
#pragma unroll
      for (int pp = 0; pp < 2; ++pp) {
        if (!c_ok[pp]) continue;
        const bool both = c_both[pp];
        f32x4 v[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          f32x4 t = acc[i][2 * pp + hf];
          t = t * rsc + bv[pp][hf];
          if (ACT == GAM_ACT_SILU) { t.x = gam_silu(t.x); t.y = gam_silu(t.y); t.z = gam_silu(t.z); t.w = gam_silu(t.w); }
          if (ACT == GAM_ACT_RELU) { t.x = fmaxf(t.x, 0.f); t.y = fmaxf(t.y, 0.f); t.z = fmaxf(t.z, 0.f); t.w = fmaxf(t.w, 0.f); }
          if (need_bt && masked) t = (f32x4){0.f, 0.f, 0.f, 0.f};
          if (scaled) t = t * g.alpha;
          if (resid) t += rv[pp][hf];
          if (tail && !both && hf == 1) t = (f32x4){0.f, 0.f, 0.f, 0.f};
          v[hf] = t;
        }
        if (guard) {
          gmax = fmaxf(gmax, fmaxf(fmaxf(fabsf(v[0].x), fabsf(v[0].y)), fmaxf(fabsf(v[0].z), fabsf(v[0].w))));
          gmax = fmaxf(gmax, fmaxf(fmaxf(fabsf(v[1].x), fabsf(v[1].y)), fmaxf(fabsf(v[1].z), fabsf(v[1].w))));
        }
        unsigned char* const cp = crow + pp * c_step;
        if (cfmt == 2) {   // plain fp16 rows (the one-term mode's operand format): 8 halfs = one 16-byte store
          const gam_half4 h0 = __builtin_convertvector(v[0], gam_half4), h1 = __builtin_convertvector(v[1], gam_half4);
          if (both) *reinterpret_cast<gam_half8*>(cp) = (gam_half8){h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
          else *reinterpret_cast<gam_half4*>(cp) = h0;
        } else if (cfmt) {   // sp32: the hi plane of the line, the lo plane 64 bytes behind it
          gam_half4 hi0, lo0, hi1, lo1;
          gam_split4(v[0], hi0, lo0);
          gam_split4(v[1], hi1, lo1);
          if (both) {
            *reinterpret_cast<gam_half8*>(cp) = (gam_half8){hi0[0], hi0[1], hi0[2], hi0[3], hi1[0], hi1[1], hi1[2], hi1[3]};
            *reinterpret_cast<gam_half8*>(cp + 64) = (gam_half8){lo0[0], lo0[1], lo0[2], lo0[3], lo1[0], lo1[1], lo1[2], lo1[3]};
          } else {
            *reinterpret_cast<gam_half4*>(cp) = hi0;
            *reinterpret_cast<gam_half4*>(cp + 64) = lo0;
          }
        } else {
          *reinterpret_cast<f32x4*>(cp) = v[0];
          if (both) *reinterpret_cast<f32x4*>(cp + 16) = v[1];
        }
      }
    }
    if (resid && i + 1 < 2 * MT) {
#pragma unroll
      for (int pp = 0; pp < 2; ++pp)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) rv[pp][hf] = rn[pp][hf];
    }
  }
  if (guard && gmax > GAM_F16_SAFE_MAX) atomicOr(g.range_flag, 1);   // bit 0 iff any stored value is beyond the limit
#undef GAM_SP_LDR
#if GAM_SP_INSTRUMENT
  if (g.tlog != nullptr) { __builtin_amdgcn_s_waitcnt(0x0070); __syncthreads(); }   // stores issued AND acknowledged by every wave
  GAM_SP_TL(3);
#endif
}

// the vectorised epilogue moves 16-byte pieces of bias / R / C rows
static inline bool gam_gemm_sp_epilogue_ok(const GamGemmArgs& a) {
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  return a.N % 4 == 0 && a.ldc % 4 == 0 && al16(a.C) && (a.bias == nullptr || al16(a.bias)) &&
         (a.R == nullptr || (a.ldr % 4 == 0 && al16(a.R)));
}

template <int ACT, int EPI, int MT, int NW, int NS = 2, bool H16 = false>
static inline void gam_launch_gemm_sp_t(const GamGemmArgs& a, int grid, hipStream_t stream) {
  static std::atomic<unsigned long long> attr_devs{0};
  constexpr int smem = GamGemmSpCfg<MT, NW, NS>::SMEM;
  static_assert(smem <= 160 * 1024, "LDS stages do not fit a CU");
  auto kern = gam_gemm_sp_kernel<ACT, EPI, MT, NW, NS, H16>;
  if (gam_set_max_lds(reinterpret_cast<const void*>(kern), smem, attr_devs) != hipSuccess) return;
  hipLaunchKernelGGL(kern, dim3(grid, a.splitk > 1 ? a.splitk : 1), dim3(128 * NW), smem, stream, a);
}

// The exact epilogue class of a launch (the GAM_EPI_* bits of its arguments as the launcher has normalised them: partial is null
// unless this is a split-K slice).  A slice stores raw sums: no other option reaches its kernel.
static inline int gam_sp_epi_bits(const GamGemmArgs& a) {
  if (a.partial != nullptr) return GAM_EPI_PART;
  return (a.c_split & GAM_EPI_CFMT) | (a.R != nullptr ? GAM_EPI_RESID : 0) | (a.alpha != 1.0f ? GAM_EPI_ALPHA : 0) |
         ((a.lens != nullptr || a.remap) ? GAM_EPI_ROWS : 0) | ((a.c_guard && a.range_flag != nullptr) ? GAM_EPI_GUARD : 0) |
         ((a.N & 7) == 4 ? GAM_EPI_TAIL : 0);
}

// Tile shape and split-K factor.  NW = 4: (64 MT) x 256 tiles, 8 waves, one workgroup per CU -- fewest bytes per FLOP.
// NW = 2: (64 MT) x 128 tiles, 4 waves, up to two workgroups per CU.  S > 1: the K range is cut into S slices (grid.y) whose
// partial sums a second pass adds up -- for grids that would leave most of the chip idle (a few utterances per GPU: the
// strong-scaling points, single clips).  The plan minimises a time model fitted to the sweep of tools/smallm_sweep.py
// (profiles/r03_smallm_sweep.txt): the busiest CU runs ceil(workgroups / slots) workgroups of
//   nk / S k-tiles x t_kt(MT, NW, sharing) + t_fix(NW, S > 1),    plus, for S > 1, the reduce pass over (S + 1) M N floats.
struct GamSpPlan { int mt, nw, s, ns; };   // tile rows / 64, tile columns / 64, split-K slices, LDS stages
// tuning hook (gam_tune_sp / GAM_SP_MT, GAM_SP_NW, GAM_SP_SPLITK): 0 = free.  Process-wide by design (a sweep tool's knob), so it
// is race-free by construction: the environment is read once (thread-safe function-local static), the fields are atomics,
// and every handle's hipGraph key carries the three values (gam_api.hip), so a plan forced after a shape was captured
// cannot replay the old tiling.
struct GamSpForce {
  std::atomic<int> mt{0}, nw{0}, s{0}, ns{0};
  GamSpForce() {
    const char* e0 = getenv("GAM_SP_MT"); const char* e1 = getenv("GAM_SP_NW"); const char* e2 = getenv("GAM_SP_SPLITK");
    const char* e3 = getenv("GAM_SP_STAGES");
    mt = e0 ? atoi(e0) : 0; nw = e1 ? atoi(e1) : 0; s = e2 ? atoi(e2) : 0; ns = e3 ? atoi(e3) : 0;
  }
};
// tile classes with a three-stage instantiation: the 4-wave tiles (128-wide) and the 128 x 256 8-wave tile (3 x 48 KB)
static inline bool gam_sp_has_ns3(int mt, int nw) { return (nw == 2 && (mt == 2 || mt == 3)) || (nw == 4 && mt == 2); }
static inline GamSpForce& gam_sp_force() { static GamSpForce f; return f; }
static inline double gam_gemm_sp_model(int M, int N, int K, int a_mode, int t, int w, int S, int ncu, int ns = 2) {
  // least-squares fit (log error) to the 810 points of profiles/r03_smallm_sweep.txt -- five layer shapes x six row counts x
  // every (MT, NW, S) -- r.m.s. 10 %, the planned configuration within 1 % of the best measured one on average (worst 11 %).
  // r04: the three-stage classes (ns = 3: one workgroup per CU whatever the tile, their LDS image is 96-144 KB) fitted to the
  // 1370-point sweep of profiles/r04_smallm_sweep_stages.txt (tools/fit_sp_model.py): r.m.s. 8 %, mean regret of the plan over
  // the 30 shapes 1.7 % (worst 12 %: M = 8032, N = 2304).
  const long wgs = (long)gam_cdiv(M, 64 * t) * gam_cdiv(N, 64 * w) * S;
  const int nkt = K / 32 / S;
  double t_kt, t_fix, rounds;
  if (ns == 3) {
    if (w == 4) { t_kt = 0.953; t_fix = S > 1 ? 6.62 : 12.8; }                 // 128 x 256, 8 waves
    else { t_kt = 0.229 * t + 0.115; t_fix = S > 1 ? 4.76 : 12.0; }            // (64 t) x 128, 4 waves
    rounds = (double)((wgs + ncu - 1) / ncu);
  } else if (w == 4) {
    t_kt = 0.335 * t + 0.425;                     // us per k-tile, one 8-wave workgroup per CU
    t_fix = S > 1 ? 6.2 : 13.2;                   // launch + prologue + epilogue (partial sums: no bias / residual / split)
    rounds = (double)((wgs + ncu - 1) / ncu);
  } else {
    const bool shared = wgs > ncu;                // two 4-wave workgroups on one CU
    const double tk_u = 0.256 * t + 0.142, tf_u = S > 1 ? 4.9 : 14.1;
    t_kt = tk_u * (shared ? 1.82 : 1.0);
    t_fix = tf_u * (shared ? 0.73 : 1.0);
    rounds = (double)((wgs + (shared ? 2 : 1) * ncu - 1) / ((shared ? 2 : 1) * ncu));
    // r06: a last round of at most ONE workgroup per CU runs unshared (756 tiles = one shared round of 512 + 244 alone): counted as a
    // whole shared round it made the three-stage class look better than it is -- the model's three worst picks (M = 8032 / N = 2304,
    // M = 12 017 / N = 1536, M = 5681 / N = 3072: 12-14 % slower than the best measured) were this; mean regret of the plan over the 36
    // shapes of profiles/r06_gemm_sweep_*.txt 1.4 % -> 0.3 %, worst 14 % -> 2 %; no pick changes at the headline's row count.
    const long cap2 = 2L * ncu, rem = wgs % cap2;
    if (shared && wgs > cap2 && rem != 0 && rem <= ncu) {
      (void)a_mode;
      double us2 = (double)(wgs / cap2) * (nkt * t_kt + t_fix) + (nkt * tk_u + tf_u);
      if (S > 1) us2 += 7.1 + (double)(S + 2) * M * N * 4.0 / 3.87e6;
      return us2;
    }
  }
  (void)a_mode;
  double us = rounds * (nkt * t_kt + t_fix);
  if (S > 1) us += 7.1 + (double)(S + 2) * M * N * 4.0 / 3.87e6;   // reduce pass: launch + partials, residual, C at ~3.9 TB/s
  return us;
}
static inline GamSpPlan gam_gemm_sp_plan(int M, int N, int K, int a_mode = 0, int ncu = 256) {
  GamSpForce& frc = gam_sp_force();
  const int f_mt = frc.mt.load(std::memory_order_relaxed), f_nw = frc.nw.load(std::memory_order_relaxed);
  int f_s = frc.s.load(std::memory_order_relaxed), f_ns = frc.ns.load(std::memory_order_relaxed);
  GamSpPlan best = {3, 4, 1, 2};
  double bt = 1e30;
  const int nk = K / 32;
  // A force this launch cannot take degrades in its own dimension only -- a split-K factor K does not divide into >= 4 whole k-tiles
  // to S = 1, three stages on the implicit-GEMM conv (two-stage tiles only) to 2 -- instead of emptying the candidate set, which left
  // the default {3, 4, 1, 2} and silently dropped a forced tile shape too.
  if (f_s > 1 && (f_s > 8 || nk % f_s != 0 || nk / f_s < 4)) f_s = 1;
  if (f_ns == 3 && a_mode != 0) f_ns = 2;
  for (int w = 4; w >= 2; w -= 2) {
    if ((f_nw == 2 || f_nw == 4) && w != f_nw) continue;
    for (int t = (w == 2 ? 3 : 4); t >= 2; --t) {
      if (f_mt >= 2 && f_mt <= 4 && t != f_mt && !(w == 2 && f_mt == 4)) continue;
      for (int S = 1; S <= 8; ++S) {
        if (f_s >= 1 && S != f_s) continue;
        if (S > 1 && (nk % S != 0 || nk / S < 4)) continue;     // whole k-tiles, and enough of them to fill the pipeline
        if (f_s < 1 && S > 1 && (long)gam_cdiv(M, 64 * t) * gam_cdiv(N, 64 * w) * 2 > ncu) continue;   // only for grids under half the chip
        for (int ns = 2; ns <= 3; ++ns) {
          if (ns == 3 && (!gam_sp_has_ns3(t, w) || a_mode != 0)) continue;   // (the implicit-GEMM conv runs the big two-stage tiles)
          if ((f_ns == 2 || f_ns == 3) && ns != f_ns && !(f_ns == 3 && !gam_sp_has_ns3(t, w))) continue;
          const double us = gam_gemm_sp_model(M, N, K, a_mode, t, w, S, ncu, ns);
          if (us < bt - 1e-9) { bt = us; best = {t, w, S, ns}; }
        }
      }
    }
  }
  return best;
}

static inline hipError_t gam_launch_gemm_sp(const GamGemmArgs& a_in, int act, hipStream_t stream) {
  GamGemmArgs a = a_in;
  if (a.M <= 0 || a.N <= 0) return hipSuccess;
  if (a.K <= 0 || a.K % 32 != 0 || a.Asp == nullptr || a.Wsp == nullptr) return hipErrorInvalidValue;
  if (a.a_mode == 0 ? (a.lda % 32 != 0) : (a.conv_c % 32 != 0)) return hipErrorInvalidValue;
  if (!gam_gemm_sp_epilogue_ok(a)) return hipErrorInvalidValue;
  // the caller made the plan (it owns the split-K workspace): a.sp_mt / a.sp_nw / a.splitk (+ a.partial when > 1)
  int mt = a.sp_mt, nw = a.sp_nw, ns = a.sp_ns;
  if (mt < 2 || mt > 4 || (nw != 2 && nw != 4) || (nw == 2 && mt == 4)) {
    const GamSpPlan p = gam_gemm_sp_plan(a.M, a.N, a.K, a.a_mode);
    mt = p.mt; nw = p.nw; ns = p.ns;
    if (a.splitk > 1 && a.partial == nullptr) return hipErrorInvalidValue;
  }
  if (ns != 3 || !gam_sp_has_ns3(mt, nw)) ns = 2;
  if (a.splitk > 1 && (a.partial == nullptr || (a.K / 32) % a.splitk != 0)) return hipErrorInvalidValue;
  if (a.n_switch > 0 && (a.Asp2 == nullptr || a.a_mode != 0 || a.n_switch % (64 * nw) != 0)) return hipErrorInvalidValue;
  if (a.splitk <= 1) { a.splitk = 0; a.partial = nullptr; }
  const int grid = gam_cdiv(a.M, 64 * mt) * gam_cdiv(a.N, 64 * nw);
  a.ntiles = grid;
#if GAM_SP_INSTRUMENT
  static long long* tl_dev = nullptr;
  static int tl_cap = 0;
  static const bool tl_on = getenv("GAM_SP_TLOG") != nullptr;   // (thread-safe one-time init)
  a.tlog = nullptr;
  if (tl_on) {
    if (grid > tl_cap) { if (tl_dev) (void)hipFree(tl_dev); (void)hipMalloc(&tl_dev, (size_t)grid * 64); tl_cap = grid; }
    (void)hipMemsetAsync(tl_dev, 0, (size_t)grid * 64, stream);
    a.tlog = tl_dev;
  }
#endif
  // tile class of the three-term kernel / of the one-term kernel (K, lda, conv_c arrive halved: gam_api.hip gemm())
#define GAM_LSP(ACTV, EPIV)                                                            \
  if (ns == 3) {                                                                       \
    if (nw == 4) gam_launch_gemm_sp_t<ACTV, EPIV, 2, 4, 3>(a, grid, stream);           \
    else if (mt == 2) gam_launch_gemm_sp_t<ACTV, EPIV, 2, 2, 3>(a, grid, stream);      \
    else gam_launch_gemm_sp_t<ACTV, EPIV, 3, 2, 3>(a, grid, stream);                   \
  } else if (nw == 2) switch (mt) {                                                    \
    case 2: gam_launch_gemm_sp_t<ACTV, EPIV, 2, 2>(a, grid, stream); break;            \
    default: gam_launch_gemm_sp_t<ACTV, EPIV, 3, 2>(a, grid, stream); break;           \
  } else switch (mt) {                                                                 \
    case 2: gam_launch_gemm_sp_t<ACTV, EPIV, 2, 4>(a, grid, stream); break;            \
    case 3: gam_launch_gemm_sp_t<ACTV, EPIV, 3, 4>(a, grid, stream); break;            \
    default: gam_launch_gemm_sp_t<ACTV, EPIV, 4, 4>(a, grid, stream); break;           \
  }
#define GAM_LSP_H16(ACTV)                                                              \
  if (ns == 3) {                                                                       \
    if (nw == 4) gam_launch_gemm_sp_t<ACTV, GAM_EPI_GENERIC, 2, 4, 3, true>(a, grid, stream);      \
    else if (mt == 2) gam_launch_gemm_sp_t<ACTV, GAM_EPI_GENERIC, 2, 2, 3, true>(a, grid, stream); \
    else gam_launch_gemm_sp_t<ACTV, GAM_EPI_GENERIC, 3, 2, 3, true>(a, grid, stream);  \
  } else if (nw == 2) {                                                                \
    if (mt == 2) gam_launch_gemm_sp_t<ACTV, GAM_EPI_GENERIC, 2, 2, 2, true>(a, grid, stream);      \
    else gam_launch_gemm_sp_t<ACTV, GAM_EPI_GENERIC, 3, 2, 2, true>(a, grid, stream);  \
  } else switch (mt) {                                                                 \
    case 2: gam_launch_gemm_sp_t<ACTV, GAM_EPI_GENERIC, 2, 4, 2, true>(a, grid, stream); break;    \
    case 3: gam_launch_gemm_sp_t<ACTV, GAM_EPI_GENERIC, 3, 4, 2, true>(a, grid, stream); break;    \
    default: gam_launch_gemm_sp_t<ACTV, GAM_EPI_GENERIC, 4, 4, 2, true>(a, grid, stream); break;   \
  }
  // The epilogue classes with an instantiation of their own = what the encoder's callers (gam_api.hip) and gam_op_gemm_ex produce in
  // the default three-term mode, one per (activation, bits) pair x the eight tile classes:
  //   none | fp32                   pointwise-conv1, the stem's Linear, linear_pos, gam_op_gemm
  //   none | fp32 + R               attention out, pointwise-conv2
  //   none | fp32 + R, alpha        FFN down
  //   none | fp32, guard            q | k | v
  //   SiLU | sp32, guard            FFN up
  //   ReLU | sp32, guard, rows      Conv2d #2 of the stem (implicit GEMM), the conv1d stem's first stage (remap)
  //   none | split-K slice          every split-K launch, whatever its activation: the reduce pass applies it
  // Anything else -- the one-term mode (fp16 C), the N % 8 == 4 tail, an activation with a residual, the conv1d stem's second stage
  // -- runs the generic class of its activation: the same code with every option read at run time.  No shape is refused for its class.
  const int epi = gam_sp_epi_bits(a);
  const int act_k = epi == GAM_EPI_PART ? GAM_ACT_NONE : act;
  enum : int { E_PLAIN = 0, E_RES = GAM_EPI_RESID, E_RESA = GAM_EPI_RESID | GAM_EPI_ALPHA, E_GRD = GAM_EPI_GUARD,
               E_UP = GAM_EPI_SP32 | GAM_EPI_GUARD, E_STEM = GAM_EPI_SP32 | GAM_EPI_GUARD | GAM_EPI_ROWS };
  if (a.h16) {
    switch (act) {
      case GAM_ACT_SILU: GAM_LSP_H16(GAM_ACT_SILU); break;
      case GAM_ACT_RELU: GAM_LSP_H16(GAM_ACT_RELU); break;
      default: GAM_LSP_H16(GAM_ACT_NONE); break;
    }
  } else if (act_k == GAM_ACT_NONE && epi == E_PLAIN) { GAM_LSP(GAM_ACT_NONE, E_PLAIN);
  } else if (act_k == GAM_ACT_NONE && epi == E_RES) { GAM_LSP(GAM_ACT_NONE, E_RES);
  } else if (act_k == GAM_ACT_NONE && epi == E_RESA) { GAM_LSP(GAM_ACT_NONE, E_RESA);
  } else if (act_k == GAM_ACT_NONE && epi == E_GRD) { GAM_LSP(GAM_ACT_NONE, E_GRD);
  } else if (act_k == GAM_ACT_SILU && epi == E_UP) { GAM_LSP(GAM_ACT_SILU, E_UP);
  } else if (act_k == GAM_ACT_RELU && epi == E_STEM) { GAM_LSP(GAM_ACT_RELU, E_STEM);
  } else if (epi == GAM_EPI_PART) { GAM_LSP(GAM_ACT_NONE, GAM_EPI_PART);
  } else {
    switch (act) {
      case GAM_ACT_SILU: GAM_LSP(GAM_ACT_SILU, GAM_EPI_GENERIC); break;
      case GAM_ACT_RELU: GAM_LSP(GAM_ACT_RELU, GAM_EPI_GENERIC); break;
      default: GAM_LSP(GAM_ACT_NONE, GAM_EPI_GENERIC); break;
    }
  }
#undef GAM_LSP
#undef GAM_LSP_H16
#if GAM_SP_INSTRUMENT
  if (tl_on) {
    std::vector<long long> t((size_t)grid * 8);
    (void)hipStreamSynchronize(stream);
    (void)hipMemcpy(t.data(), tl_dev, t.size() * 8, hipMemcpyDeviceToHost);
    long long t_first = t[0], t_last = 0;
    for (int i = 0; i < grid; ++i) { t_first = std::min(t_first, t[i * 8]); t_last = std::max(t_last, t[i * 8 + 3]); }
    auto stat = [&](auto f, const char* name) {
      std::vector<double> v(grid);
      for (int i = 0; i < grid; ++i) v[i] = f(i);
      std::sort(v.begin(), v.end());
      fprintf(stderr, "    %-26s min %7.2f  p50 %7.2f  p90 %7.2f  max %7.2f us\n", name, v[0], v[grid / 2], v[(size_t)(grid * 0.9)], v[grid - 1]);
    };
    fprintf(stderr, "[tlog] M=%d N=%d K=%d MT=%d NW=%d tiles=%d: first entry -> last exit %.2f us\n", a.M, a.N, a.K, mt, nw, grid, (t_last - t_first) * 0.01);
    stat([&](int i) { return (t[i * 8] - t_first) * 0.01; }, "entry after first entry");
    stat([&](int i) { return (t[i * 8 + 1] - t[i * 8]) * 0.01; }, "prologue (2 k-tiles land)");
    stat([&](int i) { return (t[i * 8 + 2] - t[i * 8 + 1]) * 0.01; }, "main loop");
    stat([&](int i) { return (t[i * 8 + 2] - t[i * 8 + 1]) * 0.01 / (a.K / 32); }, "  per k-tile");
    stat([&](int i) { return (double)(t[i * 8 + 6] - t[i * 8 + 5]) / std::max<long long>(1, t[i * 8 + 2] - t[i * 8 + 1]) * 100.0; }, "  shader MHz in loop");
    stat([&](int i) { return (t[i * 8 + 3] - t[i * 8 + 2]) * 0.01; }, "epilogue");
    stat([&](int i) { return (t_last - t[i * 8 + 3]) * 0.01; }, "idle after exit");
    double x_loop[8] = {0}; int x_n[8] = {0};
    for (int i = 0; i < grid; ++i) { const int x = (int)(t[i * 8 + 7] & 7); x_loop[x] += (t[i * 8 + 2] - t[i * 8 + 1]) * 0.01; ++x_n[x]; }
    fprintf(stderr, "    mean loop us by XCD:");
    for (int x = 0; x < 8; ++x) fprintf(stderr, " %.1f", x_n[x] ? x_loop[x] / x_n[x] : 0.0);
    fprintf(stderr, "\n");
  }
#endif
  return hipGetLastError();
}

// fp32 [rows, K] -> sp32 (row pitch 2*K halfs); 4 elements per thread.  rs (optional, [rows]): the row's 2^-e from
// gam_rowscale_kernel -- the values are stored multiplied by 2^e (gam_common.h gam_row_scale).
__global__ __launch_bounds__(256) void gam_to_sp32_kernel(const float* __restrict__ x, _Float16* __restrict__ y,
                                                          size_t n4, const float* __restrict__ rs, int K) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
    const size_t e = i * 4;                       // flat element index; 32-element blocks are row-aligned
    if (rs != nullptr) v = v * (1.0f / rs[e / (size_t)K]);
    gam_half4 h, l;
    gam_split4(v, h, l);
    _Float16* p = y + (e >> 5) * 64 + (e & 31);
    *reinterpret_cast<gam_half4*>(p) = h;
    *reinterpret_cast<gam_half4*>(p + 32) = l;
  }
}

// fp32 [rows, K] -> plain fp16 rows (format 2 of gam_store4; the one-term mode's operand), row-scaled like gam_to_sp32_kernel
__global__ __launch_bounds__(256) void gam_to_h16_kernel(const float* __restrict__ x, _Float16* __restrict__ y, size_t n4,
                                                         const float* __restrict__ rs, int K) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
    if (rs != nullptr) v = v * (1.0f / rs[(i * 4) / (size_t)K]);
    reinterpret_cast<gam_half4*>(y)[i] = __builtin_convertvector(v, gam_half4);
  }
}

// rs[row] = 2^-e with max|row| 2^e in [2^7, 2^8): one wave per row of an fp32 [rows, K] matrix (row pitch lda)
__global__ __launch_bounds__(256) void gam_rowscale_kernel(const float* __restrict__ x, float* __restrict__ rs, int rows,
                                                           int K, long lda) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + (size_t)row * lda;
  float m = 0.f;
  for (int k = lane; k < K; k += 64) m = fmaxf(m, fabsf(xr[k]));
  m = gam_wave_max(m);
  float s_, inv_;
  gam_row_scale(m, s_, inv_);
  if (lane == 0) rs[row] = inv_;
}
