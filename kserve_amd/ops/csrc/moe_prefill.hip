// Routed mixture-of-experts MLP for prefill-sized batches (bf16 in/out, f32
// accumulation): the contract of moe.hip (same layouts, global expert ids,
// dropped pairs, act rounded to bf16 once, output rounded once) for any
// T >= 1 with T * k <= 65536, on MFMA tiles that reuse every weight tile
// across the rows of an expert.
//
//   out[t] = bf16( sum_j topw[t][j] * down_e( bf16( silu(gate_e(x[t])) *
//                                                   up_e(x[t]) ) ) ),
//   e = topi[t][j] - expert_lo, pairs with e outside [0, E) dropped
//
// Six launches, P = T * k pairs (pair id p = t * k + j), BM = 128:
//
//   1a. count: one workgroup per block of 1024 pairs counts its pairs per
//       local expert, counts[nblk][E].
//   1b. scan (one workgroup): offsets[E + 1]; counts[b][e] becomes the first
//       sorted position of block b's pairs of expert e; the tile table: for
//       every row tile of BM sorted rows its expert and first row, and the
//       number of tiles.
//   1c. scatter: every block recomputes the stable ranks of 1a (wave ballots
//       and per-wave counters, as moe_align_kernel) and writes sorted_pair.
//       No atomic decides a position.
//   2.  gate/up grouped GEMM + SiLU*mul: workgroup = (row tile, 64
//       intermediate features). Writes act[pos][I] bf16 at the SORTED
//       position.
//   3.  down grouped GEMM: workgroup = (row tile, 128 hidden features), the
//       whole K = I in one workgroup (no split: at these sizes the tiles
//       alone fill the chip). The epilogue multiplies by topw[pair] in f32
//       and writes y[pair][H] f32 at the UNSORTED pair id.
//   4.  combine: out[t] = bf16(sum_j y[t*k + j]) in that fixed order,
//       skipping dropped pairs by re-checking topi.
//
// One tile structure serves both GEMMs. 256 threads, 4 waves as 2 (rows) x 2
// (features). LDS holds a 128 x 64 X tile and a 128 x 64 W tile, double
// buffered: 64 KB, the static limit, two workgroups per CU. In the gate/up
// GEMM the W tile is 64 gate rows followed by the 64 matching up rows of
// w_gate_up[e]; in the down GEMM it is 128 rows of w_down[e]. A wave owns 64
// tile rows and W tile rows {0, 64} + wn * 32 + [0, 32): 4 x 4 fragments of
// 16 x 16, 64 accumulator VGPRs. So in the gate/up GEMM fragments n and n + 2
// of a wave are gate and up of the same features and the activation fuses in
// registers. W is the MFMA A operand and X the B operand: a lane then holds
// 4 consecutive features of one row, and the epilogue stores 8 B (act) or
// 16 B (y) per lane and fragment.
//
// Staging: global_load_lds, 16 B per lane, 8 instructions per wave and
// K step (4 X, 4 W). The LDS write is linear; the swizzle (gemm8.hip SW = 2,
// free of bank conflicts for the fragment reads) lives in the per-lane SOURCE
// address, which is computed once before the K loop. X rows are gathered by
// those sources: tile row -> sorted position -> pair -> token (pair / k).
// Rows past the tile's count clamp to its last row; their results are never
// stored, and row fragments wholly past the count skip their MFMAs
// wave-uniformly. Only the W half of stage() and the W fragment read know how
// W is stored.
//
// K loop: stage step kt + 1, wait (counted vmcnt) for step kt, barrier,
// 16 ds_read_b128 + 32 MFMAs, barrier. The fences stay: the compiler does
// not see the LDS writes of global_load_lds.
//
// Quantized experts (weight-only fp8 and MXFP4, kserve_amd/ops/quant.py, the
// storage moe.hip takes): the GEMM kernel is a template over the weight
// format (PfBf16, PfFp8, PfMxfp4 below). X, act, the accumulators, the tile
// structure and BK = 64 do not change. W crosses HBM, L2 and LDS as codes: the
// W tile of a step is 128 rows of 64 B (fp8, 8 KB, 2 staging instructions per
// wave) or 32 B (MXFP4, 4 KB, 1 instruction). The operand layout stays: a
// lane holds 8 consecutive K of one W row, now 8 or 4 bytes, read from LDS
// with one ds_read_b64 / b32 and converted there (exactly) by the Fp8 / Mxfp4
// converts of wq_formats.h.
//
// W swizzle for those rows (wswz): a row has 4 (fp8) or 2 (MXFP4) granules of
// 16 B, and 256 B, one turn of the 64 banks, hold 4 or 8 rows; rows 4 or 8
// apart would meet on the same banks. The granule index is XORed with the
// next row bits, (row >> 2) & 3 or (row >> 3) & 1, which are offset bits 8..
// in both layouts. fp8: the 32 lanes that read one logical granule pair (16
// rows x 2 halves of a granule) then cover 16 distinct 16 B slots x 2 halves,
// every bank once. MXFP4: the 64 lanes (16 rows x 4 dwords of one granule)
// cover 8 rows x 8 dwords, every bank once. Derived for 64 banks of 4 B, not
// measured. Like the X swizzle it lives in the per-lane source address.
//
// Scales. fp8: one f32 per W row; the epilogue loads the scales of a lane's 4
// features per fragment (16 B) and multiplies the f32 accumulators, gate and
// up before SiLU*mul, down before topw. MXFP4: one E8M0 byte per W row and 32
// K, so one per row and MFMA K slice, two per row and step; the byte is the
// scale operand of that slice's convert. The bytes go through LDS (see
// stage()), requested with the step's tiles, one step ahead, and counted in
// the same wait. Per step a wave issues NW = 4 + NIW + NSC loads (8 bf16,
// 6 fp8, 6 MXFP4) and the vmcnt immediate is derived from NW.
//
// LDS: 64 KB bf16, 48 KB fp8, 42 KB MXFP4; the quantized kernels fit in 170
// registers and run three workgroups per CU, which is what the freed LDS
// buys (profiles/moe_routed.md, "Quantized prefill": 8-10% for fp8 against
// two per CU, nothing for MXFP4).
//
// Grids depend on shapes only. The row-tile dimension is the static bound
// min(cdiv(P, BM) + E, E * cdiv(T, BM)); a workgroup at or past the tile
// count exits before it touches memory. Grid order: see ks_moe_routed_
// prefill_mlp.
//
// Determinism and row independence: a row's dot products run over K in one
// fixed order whatever its tile or position (MFMA columns do not mix), and
// the combine sums in fixed order. Bit-identical from run to run; permuting
// the input rows permutes the output rows bit for bit. Not bit-equal to
// moe.hip (the K order inside a step differs).
#include "common.h"
#include "mfma_layouts.h"
#include "skinny_shared.h"
#include "tile_gemm_shared.h"
#include "wq_formats.h"

#include <type_traits>

namespace {

constexpr int BM = 128;  // rows per tile
constexpr int BK = 64;
constexpr int TILE_BYTES = 128 * BK * 2;  // one X or W tile: 16 KB
constexpr int FEAT_GATE_UP = 64;          // intermediate features per workgroup
constexpr int FEAT_DOWN = 128;            // hidden features per workgroup

constexpr int NWAVES = 4;
constexpr int ALIGN_BLOCK = 1024;  // pairs per count / scatter workgroup
constexpr int ALIGN_ROUNDS = ALIGN_BLOCK / (NWAVES * 64);
constexpr int MAX_PAIRS = 65536;
constexpr int MAX_TOPK = 8;
constexpr int MAX_EXPERTS = 256;  // local experts: 8 ballot bits, 1 thread each

// local expert of a routed id, or -1 (remote under EP, or not an expert)
__device__ __forceinline__ int local_expert(long long id, int expert_lo,
                                            int num_local) {
  const long long l = id - expert_lo;
  return (l >= 0 && l < num_local) ? (int)l : -1;
}

// ---- 1. align ----
//
// Block b holds the pairs [b * 1024, (b + 1) * 1024), wave w of it a quarter,
// in rounds of 64. A lane's rank among its wave's earlier pairs of its expert
// is the wave's running count plus the lower lanes of its match group
// (moe_align_kernel). On return wcnt[w][e] is wave w's count of expert e.
__device__ __forceinline__ void block_ranks(int (&wcnt)[NWAVES][MAX_EXPERTS],
                                            int (&le)[ALIGN_ROUNDS],
                                            int (&rank)[ALIGN_ROUNDS],
                                            const long long* __restrict__ topi,
                                            const int P, const int expert_lo,
                                            const int E) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < NWAVES * MAX_EXPERTS; i += 256)
    (&wcnt[0][0])[i] = 0;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < ALIGN_ROUNDS; ++c) {
    const int p = blockIdx.x * ALIGN_BLOCK + (wave * ALIGN_ROUNDS + c) * 64 + lane;
    int l = -1;
    if (p < P) l = local_expert(topi[p], expert_lo, E);
    unsigned long long m = __ballot(l >= 0);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (l >> b) & 1;
      const unsigned long long bb = __ballot(bit);
      m &= bit ? bb : ~bb;
    }
    le[c] = l;
    rank[c] = 0;
    if (l >= 0) {  // m = the lanes of this round with the same expert
      const int base = wcnt[wave][l];
      rank[c] = base + __popcll(m & ((1ull << lane) - 1ull));
      if ((m >> lane) == 1ull) wcnt[wave][l] = base + __popcll(m);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void prefill_count_kernel(
    int* __restrict__ counts,  // [nblk][E]
    const long long* __restrict__ topi, const int P, const int expert_lo,
    const int E) {
  __shared__ int wcnt[NWAVES][MAX_EXPERTS];
  int le[ALIGN_ROUNDS], rank[ALIGN_ROUNDS];
  block_ranks(wcnt, le, rank, topi, P, expert_lo, E);
  const int e = threadIdx.x;
  if (e < E) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) s += wcnt[w][e];
    counts[blockIdx.x * E + e] = s;
  }
}

// tiles: [0] = number of row tiles, then (expert, first sorted row) per tile
__global__ __launch_bounds__(256) void prefill_scan_kernel(
    int* __restrict__ offsets,  // [E + 1]
    int* __restrict__ counts,   // [nblk][E]: counts in, block starts out
    int* __restrict__ tiles,    // [1 + 2 * max_tiles]
    const int nblk, const int E, const int max_tiles) {
  __shared__ int total[MAX_EXPERTS];
  const int e = threadIdx.x;
  int tot = 0;
  if (e < E) {
    for (int b = 0; b < nblk; ++b) {
      const int c = counts[b * E + e];
      counts[b * E + e] = tot;
      tot += c;
    }
    total[e] = tot;
  }
  __syncthreads();
  if (e < E) {
    int run = 0, trun = 0;
    for (int i = 0; i < e; ++i) {
      run += total[i];
      trun += cdiv(total[i], BM);
    }
    offsets[e] = run;
    if (e == E - 1) offsets[E] = run + tot;
    for (int b = 0; b < nblk; ++b) counts[b * E + e] += run;
    // the bound holds when a token's experts are distinct; a routing that
    // breaks it loses rows, never writes past the table
    const int nt = cdiv(tot, BM);
    for (int i = 0; i < nt && trun + i < max_tiles; ++i) {
      tiles[1 + 2 * (trun + i)] = e;
      tiles[2 + 2 * (trun + i)] = run + i * BM;
    }
    if (e == E - 1) tiles[0] = min(trun + nt, max_tiles);
  }
}

__global__ __launch_bounds__(256) void prefill_scatter_kernel(
    int* __restrict__ sorted_pair,      // [P]
    const int* __restrict__ blk_start,  // [nblk][E]
    const long long* __restrict__ topi, const int P, const int expert_lo,
    const int E) {
  __shared__ int wcnt[NWAVES][MAX_EXPERTS];
  int le[ALIGN_ROUNDS], rank[ALIGN_ROUNDS];
  block_ranks(wcnt, le, rank, topi, P, expert_lo, E);
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int e = threadIdx.x;
  if (e < E) {  // counts -> each wave's first position
    int run = blk_start[blockIdx.x * E + e];
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
      const int c = wcnt[w][e];
      wcnt[w][e] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < ALIGN_ROUNDS; ++c)
    if (le[c] >= 0)
      sorted_pair[wcnt[wave][le[c]] + rank[c]] =
          blockIdx.x * ALIGN_BLOCK + (wave * ALIGN_ROUNDS + c) * 64 + lane;
}

// ---- 2, 3. grouped GEMMs ----

// The X and W swizzles (swz, wswz) and the expert weight formats (PfBf16,
// PfFp8, PfMxfp4) are tile_gemm_shared.h's.

// row_fast: blockIdx.x is the row tile and .y the feature block, else the
// other way round
template <class Fmt, bool GATE_UP>
__global__ __launch_bounds__(256) void moe_prefill_gemm_kernel(
    short* __restrict__ act_out,  // GATE_UP: [P][N] bf16 by sorted position
    float* __restrict__ y_out,    // !GATE_UP: [P][N] f32 by pair id
    const short* __restrict__ xin,  // GATE_UP: x [T][K]; else act [P][K]
    // GATE_UP: [E][2N] rows, else [E][N] rows, of K * ROW_BYTES / BK bytes
    const short* __restrict__ w,
    // OUT_SCALE: f32 [E][2N] / [E][N]; STEP_SCALE: E8M0 [E][2N][K/32] /
    // [E][N][K/32]; bf16: unused
    const typename Fmt::scale_t* __restrict__ scale,
    const int* __restrict__ offsets, const int* __restrict__ sorted_pair,
    const int* __restrict__ tiles, const float* __restrict__ topw,  // [P]
    const int N, const int K, const int top_k, const int row_fast) {
  constexpr int ROW_BYTES = Fmt::ROW_BYTES;
  constexpr int W_TILE_BYTES = 128 * ROW_BYTES;
  const int tile = row_fast ? blockIdx.x : blockIdx.y;
  const int fb = row_fast ? blockIdx.y : blockIdx.x;
  if (tile >= tiles[0]) return;  // unused slot of the static grid
  const int e = tiles[1 + 2 * tile];
  const int row_lo = tiles[2 + 2 * tile];
  const int rows = min(BM, offsets[e + 1] - row_lo);  // >= 1

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wm = wave >> 1;  // rows wm * 64 + [0, 64)
  const int wn = wave & 1;   // W tile rows {0, 64} + wn * 32 + [0, 32)

  // [buffer][X tile, then W tile, then MXFP4 scales: 64 dwords per wave]
  constexpr int SC_BYTES = Fmt::STEP_SCALE ? NWAVES * 256 : 0;
  __shared__ __attribute__((aligned(1024))) char
      lds[2][TILE_BYTES + W_TILE_BYTES + SC_BYTES];

  // tile row of a W tile -> row of this expert's matrix
  auto w_row_of = [&](const int r) {
    return GATE_UP ? (r >> 6) * N + fb * FEAT_GATE_UP + (r & 63)
                   : fb * FEAT_DOWN + r;
  };

  // ---- per-lane staging sources, fixed over K ----
  // Instruction ii of this wave fills the linear KB `chunk` of a tile: lane
  // writes LDS byte lin, which must hold tile byte swz(lin) (wswz for W).
  constexpr int NI = TILE_BYTES / 1024 / NWAVES;     // X: 4 per wave
  constexpr int NIW = W_TILE_BYTES / 1024 / NWAVES;  // W: 4, 2 or 1
  // W offsets count shorts in every format: a row is K * WSH / BK of them
  constexpr int WSH = ROW_BYTES / 2;
  const int w_stride = K / BK * WSH;
  const short* w_e =
      w + (long)e * (GATE_UP ? 2 : 1) * N * w_stride;  // this expert's rows
  int x_off[NI], w_off[NIW];
#pragma unroll
  for (int ii = 0; ii < NI; ++ii) {
    const int s = swz((wave + ii * NWAVES) * 1024 + lane * 16);
    const int r = s >> 7;            // tile row
    const int col = (s & 127) >> 1;  // K element inside the step
    const int pos = row_lo + min(r, rows - 1);
    const int src_row = GATE_UP ? sorted_pair[pos] / top_k : pos;
    x_off[ii] = src_row * K + col;
  }
#pragma unroll
  for (int ii = 0; ii < NIW; ++ii) {
    const int s = wswz<ROW_BYTES>((wave + ii * NWAVES) * 1024 + lane * 16);
    w_off[ii] = w_row_of(s / ROW_BYTES) * w_stride + (s % ROW_BYTES) / 2;
  }

  // MXFP4 scales go through LDS like the tiles, one 4-byte global_load_lds
  // per wave and step: lane l fetches the dword around the two E8M0 bytes
  // (one per MFMA K slice) of this step for the wave's W row l, tile row
  // wn * 32 + (l >> 5) * 64 + (l & 31). A row's bytes of a step start at an
  // even offset, so the dword is that offset rounded down to 4 (the arrays
  // are multiples of 4 bytes) and s_half says which half the step is in.
  // Loaded straight to registers the bytes would be the only VM results the
  // compiler tracks, and it then drains vmcnt to 0 before every second
  // step's converts, which ends the prefetch; LDS costs 4 ds_read_b32.
  int s_off = 0, s_half[4] = {0, 0, 0, 0};
  const unsigned char* s_e = nullptr;
  if constexpr (Fmt::STEP_SCALE) {
    s_e = reinterpret_cast<const unsigned char*>(scale) +
          (long)e * (GATE_UP ? 2 : 1) * N * (K / 32);
    s_off = w_row_of(wn * 32 + (lane >> 5) * 64 + (lane & 31)) * (K / 32);
#pragma unroll
    for (int n = 0; n < 4; ++n)  // of the row this lane converts in fragment n
      s_half[n] = (w_row_of(wn * 32 + (n >> 1) * 64 + (n & 1) * 16 +
                            (lane & 15)) * (K / 32) >> 1) & 1;
  }

  auto stage = [&](const int buf, const int kt) {
    const int k0 = kt * BK;
#pragma unroll
    for (int ii = 0; ii < NI; ++ii)
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const unsigned int*>(xin + x_off[ii] + k0),
          reinterpret_cast<unsigned int*>(
              &lds[buf][(wave + ii * NWAVES) * 1024]),
          16, 0, 0);
#pragma unroll
    for (int ii = 0; ii < NIW; ++ii)
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const unsigned int*>(w_e + w_off[ii] + kt * WSH),
          reinterpret_cast<unsigned int*>(
              &lds[buf][TILE_BYTES + (wave + ii * NWAVES) * 1024]),
          16, 0, 0);
    if constexpr (Fmt::STEP_SCALE)
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const unsigned int*>(s_e +
                                                ((s_off + kt * 2) & ~3)),
          reinterpret_cast<unsigned int*>(
              &lds[buf][TILE_BYTES + W_TILE_BYTES + wave * 256]),
          4, 0, 0);
  };
  // Per step a wave issues NW VM operations: NI X and NIW W tile loads and
  // NSC scale loads, all into LDS. Waiting for NW outstanding means the whole previous
  // step has landed. A load added to stage() is added here.
  constexpr int NSC = Fmt::STEP_SCALE ? 1 : 0;
  constexpr int NW = NI + NIW + NSC;
  constexpr int WAIT_NEXT = waitcnt_vmcnt(NW);  // one step in flight
  constexpr int WAIT_0 = waitcnt_vmcnt(0);

  // ---- fragment reads ----
  // A fragment is 16 tile rows from a multiple of 16, `base`: lane reads row
  // base + (lane & 15), granule ks * 4 + (lane >> 4). The swizzle key of
  // that row is ((lane & 15) >> 1) | (bit 4 of base) << 3, so the swizzled
  // byte is base * 128 + frag_lo[ks][bit 4 of base].
  int frag_lo[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int par = 0; par < 2; ++par)
      frag_lo[ks][par] = swz((par * 16 + (lane & 15)) * 128 +
                             (ks * 4 + (lane >> 4)) * 16) -
                         par * 16 * 128;
  // Quantized W: lane reads ROW_BYTES / 8 bytes (its 8 K) of row base +
  // (lane & 15) at byte ks * ROW_BYTES / 2 + (lane >> 4) * ROW_BYTES / 8.
  // The key comes from lane & 15 alone, so one offset serves every base.
  int wfrag_lo[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
    wfrag_lo[ks] = wswz<ROW_BYTES>((lane & 15) * ROW_BYTES +
                                   ks * (ROW_BYTES / 2) +
                                   (lane >> 4) * (ROW_BYTES / 8));

  f32x4_t acc[4][4];  // [row fragment m][W fragment n]
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // row fragments of this wave that hold a valid row: 4 in a full tile. The
  // full-tile K loop is straight-line; the ragged one skips fragments past
  // the count on a scalar branch.
  const int mact = __builtin_amdgcn_readfirstlane(
      max(0, min(4, (rows - wm * 64 + 15) >> 4)));

  auto compute = [&](const int buf, const int kt, auto full) {
    const char* xt = &lds[buf][wm * 64 * 128];
    const char* wt = &lds[buf][TILE_BYTES + wn * 32 * ROW_BYTES];
    unsigned int sc2[4];  // MXFP4: the step's two E8M0 bytes of fragment n
    if constexpr (Fmt::STEP_SCALE) {
      const unsigned int* st = reinterpret_cast<const unsigned int*>(
          &lds[buf][TILE_BYTES + W_TILE_BYTES + wave * 256]);
#pragma unroll
      for (int n = 0; n < 4; ++n)
        sc2[n] = st[(n >> 1) * 32 + (n & 1) * 16 + (lane & 15)] >>
                 (((s_half[n] + kt) & 1) * 16);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t wf[4], xf[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) {  // W tile row (n >> 1) * 64 + (n & 1) * 16
        const char* p = wt + ((n >> 1) * 64 + (n & 1) * 16) * ROW_BYTES;
        if constexpr (ROW_BYTES == 128) {
          wf[n] = *reinterpret_cast<const bf16x8_t*>(p + frag_lo[ks][n & 1]);
        } else {  // the convert; MXFP4: with the E8M0 byte of K slice ks
          float sc = 1.0f;
          if constexpr (Fmt::STEP_SCALE)
            sc = e8m0_to_float((sc2[n] >> (8 * ks)) & 0xffu);
          wf[n] = Fmt::frag(*reinterpret_cast<const typename Fmt::raw_t*>(
                                p + wfrag_lo[ks]),
                            sc);
        }
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
        xf[m] = *reinterpret_cast<const bf16x8_t*>(xt + m * 16 * 128 +
                                                   frag_lo[ks][m & 1]);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if (decltype(full)::value || m < mact) {
#pragma unroll
          for (int n = 0; n < 4; ++n)
            acc[m][n] = mfma16x16x32(wf[n], xf[m], acc[m][n]);
        }
      }
    }
  };

  const int nk = K / BK;
  auto step = [&](const int buf, const int kt, auto full) {
    if (kt + 1 < nk) {
      stage(buf ^ 1, kt + 1);
      __builtin_amdgcn_s_waitcnt(WAIT_NEXT);  // step kt landed
    } else {
      __builtin_amdgcn_s_waitcnt(WAIT_0);
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();  // raw: no vmcnt drain (counted pipeline)
    compute(buf, kt, full);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();  // readers done before lds[buf] is restaged
  };
  auto k_loop = [&](auto full) {
    stage(0, 0);
    for (int kt = 0; kt < nk; ++kt) step(kt & 1, kt, full);
  };
  if (mact == 4) k_loop(std::true_type{});
  else k_loop(std::false_type{});

  // ---- epilogue: C row = feature (lane >> 4) * 4 + reg, col = tile row ----
  // first feature of W fragment n (its tile row is the gate row in GATE_UP)
  auto feat_of = [&](const int n) {
    return GATE_UP
               ? fb * FEAT_GATE_UP + wn * 32 + (n & 1) * 16 + ((lane >> 4) << 2)
               : fb * FEAT_DOWN + (n >> 1) * 64 + wn * 32 + (n & 1) * 16 +
                     ((lane >> 4) << 2);
  };
  // OUT_SCALE: the f32 scales of the lane's four features of every
  // fragment, one 16 B load each, multiply the accumulators here, before
  // SiLU*mul and before topw
  if constexpr (Fmt::OUT_SCALE) {
    const float* s_e = scale + (long)e * (GATE_UP ? 2 : 1) * N;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const f32x4_t sc = *reinterpret_cast<const f32x4_t*>(
          s_e + (GATE_UP ? (n >> 1) * N : 0) + feat_of(n));
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m][n] *= sc;
    }
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int r = wm * 64 + m * 16 + (lane & 15);
    if (r >= rows) continue;
    const int pos = row_lo + r;
    if constexpr (GATE_UP) {
#pragma unroll
      for (int n = 0; n < 2; ++n) {  // gate in n, up in n + 2
        const int feat =
            fb * FEAT_GATE_UP + wn * 32 + n * 16 + ((lane >> 4) << 2);
        short4_t o;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const float g = acc[m][n][reg], u = acc[m][n + 2][reg];
          o[reg] = float_to_bf16_bits(g / (1.0f + __expf(-g)) * u);
        }
        *reinterpret_cast<short4_t*>(act_out + (long)pos * N + feat) = o;
      }
    } else {
      const int pair = sorted_pair[pos];
      const float tw = topw[pair];
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int feat = fb * FEAT_DOWN + (n >> 1) * 64 + wn * 32 +
                         (n & 1) * 16 + ((lane >> 4) << 2);
        *reinterpret_cast<f32x4_t*>(y_out + (long)pair * N + feat) =
            acc[m][n] * tw;
      }
    }
  }
}

// ---- 4. combine: grid (T, ceil(H / 1024)), 4 features per thread ----
// (moe_combine_kernel with one split)
__global__ __launch_bounds__(256) void prefill_combine_kernel(
    short* __restrict__ out,      // [T][H] bf16
    const float* __restrict__ y,  // [P][H]
    const long long* __restrict__ topi, const int top_k, const int H,
    const int expert_lo, const int E) {
  const int t = blockIdx.x;
  const int h = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (h >= H) return;
  float4_t s = float4_t{0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < top_k; ++j) {
    const int pair = t * top_k + j;
    if (local_expert(topi[pair], expert_lo, E) < 0) continue;
    s += *reinterpret_cast<const float4_t*>(y + (long)pair * H + h);
  }
  short4_t o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = float_to_bf16_bits(s[i]);
  *reinterpret_cast<short4_t*>(out + (long)t * H + h) = o;
}

int max_row_tiles(int T, int top_k, int E) {
  return min(cdiv(T * top_k, BM) + E, E * cdiv(T, BM));
}

}  // namespace

extern "C" int ks_moe_prefill_supported(int T, int top_k, int H, int I) {
  return T >= 1 && top_k >= 1 && top_k <= MAX_TOPK &&
         (long)T * top_k <= MAX_PAIRS && H > 0 && H % FEAT_DOWN == 0 &&
         I > 0 && I % FEAT_GATE_UP == 0;
}

// int32 workspace: offsets [E + 1], tile table [1 + 2 * max tiles], block
// starts [nblk][E], sorted_pair [P]
extern "C" long ks_moe_prefill_ws_ints(int T, int top_k, int E) {
  const int P = T * top_k;
  return (long)(E + 1) + 1 + 2 * max_row_tiles(T, top_k, E) +
         (long)cdiv(P, ALIGN_BLOCK) * E + P;
}

namespace {

// Workspaces (device): ws int32 [ks_moe_prefill_ws_ints], act bf16 [T*k][I],
// y f32 [T*k][H]. Nothing needs clearing.
//
// row_fast picks the grid order of both GEMMs: 0 = feature block fastest
// (the workgroups running together share one X tile and sweep the expert's
// weights), 1 = row tile fastest (an expert's row tiles run together and
// re-read one W tile from cache).
template <class Fmt>
hipError_t moe_routed_prefill_mlp(
    void* out, const void* x, const void* topi, const void* topw,
    const void* w_gate_up, const void* w_down, const void* gate_up_scale,
    const void* down_scale, void* ws, void* act, void* y, int T, int top_k,
    int H, int I, int E, int expert_lo, int row_fast, hipStream_t stream) {
  if (!ks_moe_prefill_supported(T, top_k, H, I) || E < 1 || E > MAX_EXPERTS)
    return hipErrorInvalidValue;
  // per-lane source offsets are 32-bit counts of elements (X) or of shorts
  // (W, never more than its elements)
  if ((long)T * H >= (1l << 31) || (long)T * top_k * I >= (1l << 31) ||
      2l * I * H >= (1l << 31))
    return hipErrorInvalidValue;
  if (((uintptr_t)x & 15) != 0 || ((uintptr_t)act & 15) != 0 ||
      ((uintptr_t)w_gate_up & 15) != 0 || ((uintptr_t)w_down & 15) != 0 ||
      ((uintptr_t)y & 15) != 0 || ((uintptr_t)out & 7) != 0 ||
      ((uintptr_t)ws & 3) != 0)
    return hipErrorInvalidValue;
  // 16 B loads of f32 scales; E8M0 rows are K / 32 bytes, an even count
  if ((Fmt::STEP_SCALE || Fmt::OUT_SCALE) &&
      (gate_up_scale == nullptr || down_scale == nullptr ||
       ((uintptr_t)gate_up_scale & 15) != 0 ||
       ((uintptr_t)down_scale & 15) != 0))
    return hipErrorInvalidValue;
  using scale_t = typename Fmt::scale_t;
  const int P = T * top_k;
  const int nblk = cdiv(P, ALIGN_BLOCK);
  const int max_tiles = max_row_tiles(T, top_k, E);
  int* offsets = (int*)ws;
  int* tiles = offsets + E + 1;
  int* blk = tiles + 1 + 2 * max_tiles;
  int* sorted_pair = blk + nblk * E;

  hipLaunchKernelGGL(prefill_count_kernel, dim3(nblk), dim3(256), 0, stream,
                     blk, (const long long*)topi, P, expert_lo, E);
  hipLaunchKernelGGL(prefill_scan_kernel, dim3(1), dim3(256), 0, stream,
                     offsets, blk, tiles, nblk, E, max_tiles);
  hipLaunchKernelGGL(prefill_scatter_kernel, dim3(nblk), dim3(256), 0, stream,
                     sorted_pair, blk, (const long long*)topi, P, expert_lo,
                     E);
  auto grid = [&](int nfb) {
    return row_fast ? dim3(max_tiles, nfb) : dim3(nfb, max_tiles);
  };
  hipLaunchKernelGGL((moe_prefill_gemm_kernel<Fmt, true>),
                     grid(I / FEAT_GATE_UP), dim3(256), 0, stream, (short*)act,
                     (float*)nullptr, (const short*)x, (const short*)w_gate_up,
                     (const scale_t*)gate_up_scale, offsets, sorted_pair,
                     tiles, (const float*)topw, I, H, top_k, row_fast);
  hipLaunchKernelGGL((moe_prefill_gemm_kernel<Fmt, false>),
                     grid(H / FEAT_DOWN), dim3(256), 0, stream, (short*)nullptr,
                     (float*)y, (const short*)act, (const short*)w_down,
                     (const scale_t*)down_scale, offsets, sorted_pair, tiles,
                     (const float*)topw, H, I, top_k, row_fast);
  hipLaunchKernelGGL(prefill_combine_kernel, dim3(T, cdiv(H, 1024)),
                     dim3(256), 0, stream, (short*)out, (const float*)y,
                     (const long long*)topi, top_k, H, expert_lo, E);
  HIP_CHECK_KERNEL();
  return hipSuccess;
}

}  // namespace

// wformat: 0 = bf16 experts (scales unused), 1 = fp8 codes [E][2I][H] /
// [E][H][I] with f32 scales [E][2I] / [E][H], 2 = MXFP4 codes [E][2I][H/2] /
// [E][H][I/2] with E8M0 scales [E][2I][H/32] / [E][H][I/32]
extern "C" hipError_t ks_moe_routed_prefill_mlp(
    void* out, const void* x, const void* topi, const void* topw,
    const void* w_gate_up, const void* w_down, const void* gate_up_scale,
    const void* down_scale, int wformat, void* ws, void* act, void* y, int T,
    int top_k, int H, int I, int E, int expert_lo, int row_fast,
    hipStream_t stream) {
#define CASE(Fmt)                                                            \
  return moe_routed_prefill_mlp<Fmt>(out, x, topi, topw, w_gate_up, w_down,  \
                                     gate_up_scale, down_scale, ws, act, y,  \
                                     T, top_k, H, I, E, expert_lo, row_fast, \
                                     stream)
  switch (wformat) {
    case 0: CASE(PfBf16);
    case 1: CASE(PfFp8);
    case 2: CASE(PfMxfp4);
  }
#undef CASE
  return hipErrorInvalidValue;
}
