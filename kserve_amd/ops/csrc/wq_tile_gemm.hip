// Weight-only quantized linear for batches above the skinny GEMM's range
// (bf16 activations, fp8 or MXFP4 weights of kserve_amd/ops/quant.py, f32
// accumulation): the weight crosses HBM, L2 and LDS once, as codes, and is
// converted (exactly, wq_formats.h) where the MFMA fragment is read.
//
//   out[n][m] = bf16( scale_m * sum_k x[n][k] * code[m][k] + bias[m] )
//
// scale_m is the f32 row scale of fp8; MXFP4's E8M0 block scale is applied
// inside the convert instead. bias (bf16 [M], may be null) is added in f32
// before the one rounding. Any N >= 1, M % 64 == 0, K % 64 == 0 (fp8) or
// K % 128 == 0 (MXFP4); x rows may be strided (stride % 8 == 0).
//
// Tile structure: moe_prefill.hip's, without the gather. 256 threads, 4 waves
// as 2 (token rows) x 2 (features); a workgroup owns 128 tokens x 128
// features of one K range and walks it in steps of BK = 64. W is the MFMA A
// operand and X the B operand (v_mfma_f32_16x16x32_bf16), so a lane holds 4
// consecutive features of one token and stores 8 B (bf16) or 16 B (f32
// partial) per fragment. A wave owns 64 token rows and W tile rows {0, 64} +
// wn * 32 + [0, 32): 4 x 4 fragments, 64 accumulator VGPRs.
//
// Staging: global_load_lds, 16 B per lane, double buffered. Per step the X
// tile is 128 rows of 128 B (16 KB, source row x + n * stride) and the W tile
// 128 rows of 64 B (fp8, 8 KB) or 32 B (MXFP4, 4 KB) plus, for MXFP4, one
// dword per W row holding the step's two E8M0 bytes. The LDS write is linear;
// the swizzles (swz for X, wswz for W, tile_gemm_shared.h) live in the
// per-lane SOURCE address, computed once before the K loop. LDS: 48 KB fp8,
// 42 KB MXFP4.
//
// K loop: stage step kt + 1, wait (counted vmcnt) for step kt, barrier,
// fragment reads + converts + 32 MFMAs, barrier. Per step a wave issues
// NW = 4 (X) + NIW (W: 2 fp8, 1 MXFP4) + NSC (MXFP4 scales: 1) loads, all
// into LDS, and the vmcnt immediate is derived from NW.
//
// Ragged edges: token rows past N clamp their source to row N - 1 and are
// never stored; row fragments wholly past N skip their MFMAs wave-uniformly.
// When M is a multiple of 64 but not of 128, the upper 64 W rows of the last
// feature tile clamp to row M - 1, their fragments (n = 2, 3 of every wave)
// are skipped the same way and never stored.
//
// Split-K: S in {1, 2, 4, 8} K ranges of K / (64 S) whole steps each. S is a
// function of (M, K) only (ks_wq_tile_nsplit), never of N: a row's sum order
// does not depend on the batch it sits in. S = 1: the epilogue scales, adds
// the bias and rounds in registers. S > 1: the GEMM writes f32 partials
// [S][N][M] and wq_tile_reduce_kernel sums them in split order, scales, adds
// the bias and rounds once. No atomics: bit-identical from run to run.
//
// Grid: one dimension, cdiv(N, 128) * cdiv(M, 128) * S workgroups, remapped
// at the top of the kernel. Assuming consecutive workgroup ids go round-robin
// over the 8 XCDs, id -> (id % 8) * (ids per XCD) + id / 8 gives every XCD a
// contiguous run of logical indices, and the row tile is the fastest logical
// digit: all row tiles of one (feature tile, split) run back to back on one
// XCD, so a W tile leaves HBM once and is re-read from that XCD's L2.
// plain_order = 1 keeps id as the logical index (tools/gemm_bench.py
// --wq-tile measures both). Measured (profiles/wq_tile_gemm.md): up to 512
// tokens, the range ops dispatches here, neither is the faster one (mixed,
// mostly inside the spread; under 2.5 % apart summed over the four Llama-3-8B
// shapes; the plain order ahead by 13-16 % on o at 256 tokens), so the
// designed order stays; from 2048 tokens the plain order wins (13-25 % at
// 4096), where X is the larger stream.
//
// Grids depend on shapes only and nothing synchronises with the host: the
// launches capture into a hipGraph.
#include "common.h"
#include "mfma_layouts.h"
#include "skinny_shared.h"
#include "tile_gemm_shared.h"
#include "wq_formats.h"

#include <type_traits>

namespace {

constexpr int BM = 128;  // token rows per tile
constexpr int BN = 128;  // features per tile
constexpr int BK = 64;
constexpr int X_TILE_BYTES = BM * BK * 2;  // 16 KB
constexpr int NWAVES = 4;
constexpr int NUM_XCD = 8;

template <class Fmt, bool SPLIT>
__global__ __launch_bounds__(256) void wq_tile_gemm_kernel(
    short* __restrict__ out,    // !SPLIT: [N][M] bf16
    float* __restrict__ part,   // SPLIT: [S][N][M] f32
    const short* __restrict__ x,  // [N] rows of K bf16, x_stride apart
    const short* __restrict__ w,  // [M] rows of K * ROW_BYTES / BK bytes
    // OUT_SCALE: f32 [M]; STEP_SCALE: E8M0 [M][K/32]
    const typename Fmt::scale_t* __restrict__ scale,
    const short* __restrict__ bias,  // bf16 [M] or null; !SPLIT only
    const int N, const int M, const int K, const int x_stride,
    const int nk_split,  // K steps per split
    const int plain_order) {
  constexpr int ROW_BYTES = Fmt::ROW_BYTES;
  constexpr int W_TILE_BYTES = BN * ROW_BYTES;

  // ---- workgroup id -> (row tile, feature tile, split) ----
  const int n_rt = cdiv(N, BM);
  const int n_fb = cdiv(M, BN);
  int L = blockIdx.x;
  if (!plain_order) {
    const int per = gridDim.x / NUM_XCD, rem = gridDim.x % NUM_XCD;
    const int xcd = L % NUM_XCD;
    L = xcd * per + min(xcd, rem) + L / NUM_XCD;
  }
  const int rt = L % n_rt;
  const int fb = (L / n_rt) % n_fb;
  const int split = L / n_rt / n_fb;
  const int rows = min(BM, N - rt * BM);   // >= 1
  const int wrows = min(BN, M - fb * BN);  // 64 or 128

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wm = wave >> 1;  // token rows wm * 64 + [0, 64)
  const int wn = wave & 1;   // W tile rows {0, 64} + wn * 32 + [0, 32)

  // [buffer][X tile, then W tile, then MXFP4 scales: 64 dwords per wave]
  constexpr int SC_BYTES = Fmt::STEP_SCALE ? NWAVES * 256 : 0;
  __shared__ __attribute__((aligned(1024))) char
      lds[2][X_TILE_BYTES + W_TILE_BYTES + SC_BYTES];

  // tile row of the W tile -> row of the matrix, clamped at the half tile
  auto w_row_of = [&](const int r) { return fb * BN + min(r, wrows - 1); };

  // ---- per-lane staging sources, fixed over K ----
  // Instruction ii of this wave fills the linear KB `chunk` of a tile: lane
  // writes LDS byte lin, which must hold tile byte swz(lin) (wswz for W).
  constexpr int NI = X_TILE_BYTES / 1024 / NWAVES;   // X: 4 per wave
  constexpr int NIW = W_TILE_BYTES / 1024 / NWAVES;  // W: 2 or 1
  // W offsets count shorts in both formats: a row is K * WSH / BK of them
  constexpr int WSH = ROW_BYTES / 2;
  const int w_stride = K / BK * WSH;
  int x_off[NI], w_off[NIW];
#pragma unroll
  for (int ii = 0; ii < NI; ++ii) {
    const int s = swz((wave + ii * NWAVES) * 1024 + lane * 16);
    const int r = s >> 7;            // tile row
    const int col = (s & 127) >> 1;  // K element inside the step
    x_off[ii] = (rt * BM + min(r, rows - 1)) * x_stride + col;
  }
#pragma unroll
  for (int ii = 0; ii < NIW; ++ii) {
    const int s = wswz<ROW_BYTES>((wave + ii * NWAVES) * 1024 + lane * 16);
    w_off[ii] = w_row_of(s / ROW_BYTES) * w_stride + (s % ROW_BYTES) / 2;
  }

  // MXFP4 scales go through LDS like the tiles (moe_prefill.hip has the
  // reason), one 4-byte global_load_lds per wave and step: lane l fetches
  // the dword around the step's two E8M0 bytes of the wave's W row l, tile
  // row wn * 32 + (l >> 5) * 64 + (l & 31). K % 128 == 0 makes a row's
  // K / 32 bytes a multiple of 4, so the dword of step kt starts at byte
  // (kt * 2) & ~3 of the row and the step's half of it is kt & 1.
  int s_off = 0;
  const unsigned char* s_base = nullptr;
  if constexpr (Fmt::STEP_SCALE) {
    s_base = reinterpret_cast<const unsigned char*>(scale);
    s_off = w_row_of(wn * 32 + (lane >> 5) * 64 + (lane & 31)) * (K / 32);
  }

  auto stage = [&](const int buf, const int kt) {
    const int k0 = kt * BK;
#pragma unroll
    for (int ii = 0; ii < NI; ++ii)
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const unsigned int*>(x + x_off[ii] + k0),
          reinterpret_cast<unsigned int*>(
              &lds[buf][(wave + ii * NWAVES) * 1024]),
          16, 0, 0);
#pragma unroll
    for (int ii = 0; ii < NIW; ++ii)
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const unsigned int*>(w + w_off[ii] + kt * WSH),
          reinterpret_cast<unsigned int*>(
              &lds[buf][X_TILE_BYTES + (wave + ii * NWAVES) * 1024]),
          16, 0, 0);
    if constexpr (Fmt::STEP_SCALE)
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const unsigned int*>(s_base + s_off +
                                                ((kt * 2) & ~3)),
          reinterpret_cast<unsigned int*>(
              &lds[buf][X_TILE_BYTES + W_TILE_BYTES + wave * 256]),
          4, 0, 0);
  };
  // Per step a wave issues NW VM operations: NI X and NIW W tile loads and
  // NSC scale loads, all into LDS. Waiting for NW outstanding means the whole
  // previous step has landed. A load added to stage() is added here.
  constexpr int NSC = Fmt::STEP_SCALE ? 1 : 0;
  constexpr int NW = NI + NIW + NSC;
  constexpr int WAIT_NEXT = waitcnt_vmcnt(NW);  // one step in flight
  constexpr int WAIT_0 = waitcnt_vmcnt(0);

  // ---- fragment reads (moe_prefill.hip) ----
  // X: 16 tile rows from a multiple of 16, `base`: lane reads row base +
  // (lane & 15), granule ks * 4 + (lane >> 4); the swizzled byte is
  // base * 128 + xfrag_lo[ks][bit 4 of base].
  int xfrag_lo[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int par = 0; par < 2; ++par)
      xfrag_lo[ks][par] = swz((par * 16 + (lane & 15)) * 128 +
                              (ks * 4 + (lane >> 4)) * 16) -
                          par * 16 * 128;
  // W: lane reads ROW_BYTES / 8 bytes (its 8 K) of row base + (lane & 15) at
  // byte ks * ROW_BYTES / 2 + (lane >> 4) * ROW_BYTES / 8. The key comes
  // from lane & 15 alone, so one offset serves every base.
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

  // fragments of this wave that hold a valid token row (of 4) and a valid W
  // row (2 in a half tile, else 4). The full-tile K loop is straight-line;
  // the ragged one skips the others on scalar branches.
  const int mact = __builtin_amdgcn_readfirstlane(
      max(0, min(4, (rows - wm * 64 + 15) >> 4)));
  const int nact = wrows > 64 ? 4 : 2;

  auto compute = [&](const int buf, const int kt, auto full) {
    const char* xt = &lds[buf][wm * 64 * 128];
    const char* wt = &lds[buf][X_TILE_BYTES + wn * 32 * ROW_BYTES];
    unsigned int sc2[4];  // MXFP4: the step's two E8M0 bytes of fragment n
    if constexpr (Fmt::STEP_SCALE) {
      const unsigned int* st = reinterpret_cast<const unsigned int*>(
          &lds[buf][X_TILE_BYTES + W_TILE_BYTES + wave * 256]);
#pragma unroll
      for (int n = 0; n < 4; ++n)
        sc2[n] = st[(n >> 1) * 32 + (n & 1) * 16 + (lane & 15)] >>
                 ((kt & 1) * 16);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t wf[4], xf[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) {  // W tile row (n >> 1) * 64 + (n & 1) * 16
        const char* p = wt + ((n >> 1) * 64 + (n & 1) * 16) * ROW_BYTES;
        float sc = 1.0f;  // MXFP4: the E8M0 byte of K slice ks
        if constexpr (Fmt::STEP_SCALE)
          sc = e8m0_to_float((sc2[n] >> (8 * ks)) & 0xffu);
        wf[n] = Fmt::frag(
            *reinterpret_cast<const typename Fmt::raw_t*>(p + wfrag_lo[ks]),
            sc);
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
        xf[m] = *reinterpret_cast<const bf16x8_t*>(xt + m * 16 * 128 +
                                                   xfrag_lo[ks][m & 1]);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if (decltype(full)::value || m < mact) {
#pragma unroll
          for (int n = 0; n < 4; ++n)
            if (decltype(full)::value || n < nact)
              acc[m][n] = mfma16x16x32(wf[n], xf[m], acc[m][n]);
        }
      }
    }
  };

  const int kt_lo = split * nk_split, kt_hi = kt_lo + nk_split;
  auto step = [&](const int buf, const int kt, auto full) {
    if (kt + 1 < kt_hi) {
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
    stage(0, kt_lo);
    for (int kt = kt_lo; kt < kt_hi; ++kt) step((kt - kt_lo) & 1, kt, full);
  };
  if (mact == 4 && nact == 4) k_loop(std::true_type{});
  else k_loop(std::false_type{});

  // ---- epilogue: C row = feature (lane >> 4) * 4 + reg, col = token row ----
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    if (n >= nact) continue;
    const int feat =
        fb * BN + (n >> 1) * 64 + wn * 32 + (n & 1) * 16 + ((lane >> 4) << 2);
    f32x4_t sc = f32x4_t{1.f, 1.f, 1.f, 1.f};
    f32x4_t b = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if constexpr (!SPLIT) {
      if constexpr (Fmt::OUT_SCALE)
        sc = *reinterpret_cast<const f32x4_t*>(scale + feat);
      if (bias != nullptr) {
        const short4_t bb = *reinterpret_cast<const short4_t*>(bias + feat);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) b[reg] = bf16_bits_to_float(bb[reg]);
      }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int r = wm * 64 + m * 16 + (lane & 15);
      if (r >= rows) continue;
      const long tok = rt * BM + r;
      if constexpr (SPLIT) {
        *reinterpret_cast<f32x4_t*>(part + ((long)split * N + tok) * M +
                                    feat) = acc[m][n];
      } else {
        short4_t o;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          o[reg] = float_to_bf16_bits(acc[m][n][reg] * sc[reg] + b[reg]);
        *reinterpret_cast<short4_t*>(out + tok * M + feat) = o;
      }
    }
  }
}

// out[n][m] = bf16(scale[m] * sum_s part[s][n][m] + bias[m]), 4 features per
// thread, the sum in split order. scale (f32 [M]) and bias (bf16 [M]) may be
// null.
__global__ __launch_bounds__(256) void wq_tile_reduce_kernel(
    short* __restrict__ out, const float* __restrict__ part,
    const float* __restrict__ scale, const short* __restrict__ bias,
    const long nm, const int M, const int S) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= nm) return;
  const int m = (int)(i % M);
  f32x4_t s = *reinterpret_cast<const f32x4_t*>(part + i);
  for (int sp = 1; sp < S; ++sp)
    s += *reinterpret_cast<const f32x4_t*>(part + sp * nm + i);
  if (scale != nullptr) s *= *reinterpret_cast<const f32x4_t*>(scale + m);
  short4_t o;
  short4_t bb = short4_t{0, 0, 0, 0};
  if (bias != nullptr) bb = *reinterpret_cast<const short4_t*>(bias + m);
#pragma unroll
  for (int reg = 0; reg < 4; ++reg)
    o[reg] = float_to_bf16_bits(s[reg] + bf16_bits_to_float(bb[reg]));
  *reinterpret_cast<short4_t*>(out + i) = o;
}

template <class Fmt>
hipError_t wq_tile_gemm(void* out, void* part, const void* x, const void* w,
                        const void* scale, const void* bias, int M, int K,
                        int N, long x_stride, int S, int plain_order,
                        hipStream_t stream) {
  using scale_t = typename Fmt::scale_t;
  const int nk = K / BK;
  const int grid = cdiv(N, BM) * cdiv(M, BN) * S;
  const float* out_scale = Fmt::OUT_SCALE ? (const float*)scale : nullptr;
  if (S == 1) {
    hipLaunchKernelGGL((wq_tile_gemm_kernel<Fmt, false>), dim3(grid),
                       dim3(256), 0, stream, (short*)out, (float*)nullptr,
                       (const short*)x, (const short*)w,
                       (const scale_t*)scale, (const short*)bias, N, M, K,
                       (int)x_stride, nk, plain_order);
  } else {
    hipLaunchKernelGGL((wq_tile_gemm_kernel<Fmt, true>), dim3(grid),
                       dim3(256), 0, stream, (short*)nullptr, (float*)part,
                       (const short*)x, (const short*)w,
                       (const scale_t*)scale, (const short*)nullptr, N, M, K,
                       (int)x_stride, nk / S, plain_order);
    const long nm = (long)N * M;
    hipLaunchKernelGGL(wq_tile_reduce_kernel, dim3((int)((nm / 4 + 255) / 256)),
                       dim3(256), 0, stream, (short*)out, (const float*)part,
                       out_scale, (const short*)bias, nm, M, S);
  }
  HIP_CHECK_KERNEL();
  return hipSuccess;
}

}  // namespace

// K splits of an [M][K] weight: double S while the feature tiles times S
// leave the chip short of work at two row tiles (fewer than 128 groups on
// 256 CUs), every split keeps a whole number of K steps and at least two of
// them. A function of the weight alone, so a row's sum order never depends
// on its batch. profiles/wq_tile_gemm.md has the forced-split measurements.
extern "C" int ks_wq_tile_nsplit(int M, int K) {
  const int nk = K / BK;
  const int n_fb = cdiv(M, BN);
  int S = 1;
  while (S < 8 && n_fb * S < 128 && nk % (2 * S) == 0 && nk / (2 * S) >= 2)
    S *= 2;
  return S;
}

// wformat: 1 = fp8 codes [M][K] with f32 scales [M], 2 = MXFP4 codes
// [M][K/2] with E8M0 scales [M][K/32]. n_splits in {1, 2, 4, 8} dividing
// K / 64; part is f32 [n_splits][N][M] (unused at 1). bias bf16 [M] or null.
extern "C" hipError_t ks_wq_tile_gemm(void* out, void* part, const void* x,
                                      const void* qweight, const void* scale,
                                      const void* bias, int wformat, int M,
                                      int K, int N, long x_stride,
                                      int n_splits, int plain_order,
                                      hipStream_t stream) {
  const int k_multiple = wformat == 2 ? 128 : BK;
  if (N < 1 || M < 64 || M % 64 != 0 || K < k_multiple ||
      K % k_multiple != 0 || x_stride < K || x_stride % 8 != 0)
    return hipErrorInvalidValue;
  if (n_splits != 1 && n_splits != 2 && n_splits != 4 && n_splits != 8)
    return hipErrorInvalidValue;
  if ((K / BK) % n_splits != 0) return hipErrorInvalidValue;
  // per-lane source offsets are 32-bit counts of elements (X) or of shorts
  // (W, never more than its elements); so are the workgroup counts of the
  // GEMM and of the reduce (N * M / 1024)
  if ((long)N * x_stride >= (1l << 31) || (long)M * K >= (1l << 31) ||
      (long)N * M >= (1l << 31) ||
      (long)cdiv(N, BM) * cdiv(M, BN) * n_splits >= (1l << 31))
    return hipErrorInvalidValue;
  if (((uintptr_t)x & 15) != 0 || ((uintptr_t)qweight & 15) != 0 ||
      ((uintptr_t)out & 7) != 0 || ((uintptr_t)bias & 7) != 0 ||
      scale == nullptr || ((uintptr_t)scale & 15) != 0)
    return hipErrorInvalidValue;
  if (n_splits > 1 && (part == nullptr || ((uintptr_t)part & 15) != 0))
    return hipErrorInvalidValue;
  switch (wformat) {
    case 1:
      return wq_tile_gemm<PfFp8>(out, part, x, qweight, scale, bias, M, K, N,
                                 x_stride, n_splits, plain_order, stream);
    case 2:
      return wq_tile_gemm<PfMxfp4>(out, part, x, qweight, scale, bias, M, K, N,
                                   x_stride, n_splits, plain_order, stream);
  }
  return hipErrorInvalidValue;
}
