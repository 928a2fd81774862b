// Weight-only quantized decode GEMM (bf16 activations) and row dequantizers,
// one kernel for two weight formats:
//
//   fp8 (OCP E4M3, one f32 scale per output feature, W8A16)
//     ks_skinny_gemm_w8:   out[N][M] bf16 = (x[N][K] bf16 @ q[M][K]^T fp8) * scale[M]
//     ks_dequant_fp8_rows: out[M][K] bf16 = bf16_rne(float(q[M][K]) * scale[M])
//   MXFP4 (OCP E2M1 + one E8M0 scale per 32 elements of a row, W4A16)
//     ks_skinny_gemm_w4:     out[N][M] bf16 = x[N][K] bf16 @ dequant(q, s)[M][K]^T
//     ks_dequant_mxfp4_rows: out[M][K] bf16 = e2m1(q[M][K/2]) * 2^(s[M][K/32]-127)
//
// Stored MXFP4 (kserve_amd/ops/quant.py): byte i of a row holds element 2i
// in bits 3:0 and element 2i+1 in bits 7:4.
//
// The GEMM keeps skinny_gemm.hip's structure (4 waves x 16 features, X tile
// shared through LDS with pre-swizzled global_load_lds sources, counted-vmcnt
// double buffer with raw s_barrier, NT template over token tiles, K-split
// into disjoint bf16 partials + a reduce kernel). What changes is the W
// side: every W row is read by exactly one wave, so W never goes through
// LDS. Each lane loads 16 consecutive bytes of its feature row straight into
// registers (one global_load_dwordx4 per step, prefetched one step ahead like
// the X tile), converts them in registers (exact in both formats) and feeds
// v_mfma_f32_16x16x32_bf16.
//
// Those 16 B are 16 K in fp8 and 32 K in MXFP4 (the fp8 kernel lost byte
// rate by halving the bytes in flight per load, profiles/w8_gemm.md), so a
// wave's four lane groups cover BK = 64 or 128 per step and a step is
// KK = 2 or 4 MFMAs per token tile. The fp8 per-channel scale multiplies the
// f32 accumulator in the epilogue, after the K reduction (before the bf16
// partial is written in the split-K variant). The 16 B of MXFP4 are exactly
// one MX block: the lane loads one scale byte per step and applies it inside
// the convert, so there is no scale in the epilogue. Either way the only
// approximation is the one-time weight rounding.
//
// K order: lane (kgrp = lane >> 4) holds W elements K = k0 + kgrp*(BK/4) +
// [0, BK/4); MFMA kk in [0, KK) consumes elements kk*8..kk*8+7 of them, i.e.
// X chunk (8 bf16) kc = kgrp*KK + kk. MFMA only needs A and B to agree on
// which K sits in which (lane, j) slot, so the X fragment simply reads that
// chunk.
#include "common.h"
#include "mfma_layouts.h"
#include "skinny_shared.h"

namespace {

constexpr int FEAT_PER_WAVE = 16;
constexpr int NWAVES = 4;  // 64 features per workgroup

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

// ---- the two formats: everything the kernel does differently ----
//
// BK           K per stage step; an X tile row is BK/8 chunks of 8 bf16
// KK           MFMAs per step per token tile
// K_PER_BYTE   K elements in one W byte
// scale_t      element type of the scale array
// STEP_SCALE   a lane loads one scale byte per step (row of K/32 bytes)
//              and the convert applies it
// OUT_SCALE    the epilogue multiplies by scale[feature]
// MAX_N        most tokens; the launcher's NT switch stops there
// chunk_perm   the format's part of the X tile swizzle
// cvt8         8 W elements of a lane's 16 B (MFMA kk) -> 8 bf16, element
//              order = storage order

struct Fp8 {
  static constexpr int BK = 64;
  static constexpr int KK = 2;
  static constexpr int K_PER_BYTE = 1;
  using scale_t = float;
  static constexpr bool STEP_SCALE = false;
  static constexpr bool OUT_SCALE = true;
  static constexpr int MAX_N = 256;

  // chunk = 8 bf16 = 16 B, row = 8 chunks = 128 B. One ds_read_b128 serves
  // lanes of two adjacent kgrp values together (e.g. lanes 0-3,12-15 with
  // 20-27), which here read chunks kc and kc^2; the skinny_gemm swizzle
  // kc ^ (row & 7) would put both on the same bank parity (2-way conflict).
  // Folding bit 1 of kc into bit 0 first makes the two chunk positions
  // differ in parity, so the 16 lanes of a group cover 16 distinct 4-bank
  // slots. chunk_perm is an involution (bit 1 is kept).
  static __device__ __forceinline__ int chunk_perm(int kc) {
    return kc ^ ((kc >> 1) & 1);
  }

  // two dwords of fp8 bytes; E4M3 fits bf16's mantissa
  static __device__ __forceinline__ bf16x8_t cvt8(const u32x4_t& w, int kk,
                                                  float) {
    const unsigned int lo = w[kk * 2], hi = w[kk * 2 + 1];
    const bf16x2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
    const bf16x2_t p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
    const bf16x2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
    const bf16x2_t p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
    return bf16x8_t{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
  }
};

struct Mxfp4 {
  static constexpr int BK = 128;
  static constexpr int KK = 4;
  static constexpr int K_PER_BYTE = 2;
  using scale_t = unsigned char;
  static constexpr bool STEP_SCALE = true;
  static constexpr bool OUT_SCALE = false;
  static constexpr int MAX_N = 128;  // the X tile fills 64 KB of LDS there

  // The hardware convert reads the byte's bits 3:0 as the first element of
  // the pair, which is the stored order. Were it the other way round, the
  // fix is in registers (swap the nibbles of every byte), not in the format.
  static constexpr bool SWAP_NIBBLES = false;

  // chunk = 8 bf16 = 16 B, row = 16 chunks = 256 B = one full LDS bank row,
  // so the slot (4 banks) of a chunk is its position in the row.
  //
  // Derived (from the ds_read_b128 lane groups, not measured): one
  // ds_read_b128 serves 16 lanes that are 8 lanes of an even kgrp and 8 of
  // the next odd one: token rows m in S = {0-3,12-15} of one and
  // S' = {4-11} of the other. They read chunks kc and kc^4 (kc = kgrp*4+kk).
  // S is the subgroup {m : bit2 == bit3} and S' its coset. A plain
  // kc ^ (row & 15) puts the 8 rows of one kgrp on 8 distinct slots, but the
  // two kgrps land on the SAME 8 slots (kc^S == (kc^4)^S'): a 2-way
  // conflict. Folding bit 2 of kc into bit 3 first makes bit2^bit3 of the
  // permuted chunk independent of bit 2 of kc, so the two halves fall in
  // different cosets and the 16 lanes cover all 16 slots. chunk_perm is an
  // involution (bit 2 is kept). Fp8's perm (bit 1 into bit 0) is the same
  // argument for its 8-chunk rows and does not separate these.
  static __device__ __forceinline__ int chunk_perm(int kc) {
    return kc ^ ((kc & 4) << 1);
  }

  // one dword of fp4 nibbles, times the block scale (a power of two)
  static __device__ __forceinline__ bf16x8_t cvt8(const u32x4_t& w, int kk,
                                                  const float sc) {
    unsigned int v = w[kk];
    if constexpr (SWAP_NIBBLES)
      v = ((v & 0x0f0f0f0fu) << 4) | ((v >> 4) & 0x0f0f0f0fu);
    const bf16x2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 0);
    const bf16x2_t p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 1);
    const bf16x2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 2);
    const bf16x2_t p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 3);
    return bf16x8_t{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
  }
};

// E8M0 code -> the f32 with that biased exponent (2^(c-127))
__device__ __forceinline__ float e8m0_to_float(unsigned int c) {
  return __uint_as_float(c << 23);
}

// what one K-step of W occupies in a lane's registers
template <bool STEP_SCALE>
struct WRegs {
  u32x4_t w;
};
template <>
struct WRegs<true> {
  u32x4_t w;
  unsigned int s;
};

template <class Fmt, int NT, bool SPLIT>
__global__ __launch_bounds__(256) void skinny_gemm_wq_kernel(
    short* __restrict__ out,      // [N][M] bf16 (!SPLIT)
    short* __restrict__ out_ws,   // [nsplit][N][M] bf16 partials (SPLIT)
    const short* __restrict__ x,  // [N][K] row stride xs
    const unsigned char* __restrict__ w,  // [M][K / K_PER_BYTE] codes
    const typename Fmt::scale_t* __restrict__ scale,  // [M] or [M][K/32]
    const int M, const int K, const int N, const long xs,
    const int k_per_split) {
  constexpr int BK = Fmt::BK;
  constexpr int ROW_CHUNKS = BK / 8;  // 16 B chunks in an X tile row
  using Regs = WRegs<Fmt::STEP_SCALE>;

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int f_base = blockIdx.x * (NWAVES * FEAT_PER_WAVE);
  const int k_lo = blockIdx.y * k_per_split;
  const int k_hi = min(K, k_lo + k_per_split);

  // LDS: double-buffered X tile [NT*16][BK], swizzled. A tile is NINSTR
  // wg-wide 1 KB instructions; where that is no multiple of the wave count
  // (fp8 with odd NT) the last round is padded so that every wave issues
  // exactly NI of them, and the padding lands in a 1 KB dump slot.
  constexpr int NINSTR = NT * 16 * ROW_CHUNKS / 64;
  constexpr int NI = (NINSTR + NWAVES - 1) / NWAVES;  // per wave per step
  constexpr bool PAD = NINSTR % NWAVES != 0;
  constexpr int TILE_SHORTS = NT * 16 * BK;
  __shared__ short tile[2][TILE_SHORTS];

  f32x4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int m_local = lane & 15;
  const int kgrp = lane >> 4;
  // this lane's W stream: its feature row, 16 bytes per K-step, and with
  // STEP_SCALE the scale byte of that block
  const long frow = f_base + wave * FEAT_PER_WAVE + m_local;
  const unsigned char* wrow = w + frow * (K / Fmt::K_PER_BYTE) + kgrp * 16;
  const unsigned char* srow = nullptr;
  if constexpr (Fmt::STEP_SCALE)
    srow = scale + frow * (K / 32) + kgrp;

  auto lds_row_idx = [](int row, int kc) {
    return (row * ROW_CHUNKS +
            (Fmt::chunk_perm(kc) ^ (row & (ROW_CHUNKS - 1)))) * 8;  // shorts
  };

  // stage the X BK-slice at k-offset k0 into buf
  auto stage = [&](int buf, int k0) {
#pragma unroll
    for (int ii = 0; ii < NI; ++ii) {
      const int i = wave + ii * NWAVES;
      const int g = i * 64 + lane;
      const short* src;
      short* dst;
      if (!PAD || i < NINSTR) {
        dst = &tile[buf][i * 64 * 8];
        int row = g / ROW_CHUNKS;  // token row
        const int kc_src = Fmt::chunk_perm((g & (ROW_CHUNKS - 1)) ^
                                           (row & (ROW_CHUNKS - 1)));
        if (row >= N) row = N - 1;  // clamp padded token rows
        src = x + (long)row * xs + (kc_src << 3) + k0;
      } else {  // padding instr keeps per-wave vmcnt uniform
        __shared__ short dump[512];
        dst = dump;
        src = x;
      }
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const unsigned int*>(src),
          reinterpret_cast<unsigned int*>(dst), 16, 0, 0);
    }
  };
  // this lane's W bytes (and scale byte) of the step at k0 -> registers
  auto load_w = [&](Regs& r, int k0) {
    r.w = *reinterpret_cast<const u32x4_t*>(wrow + k0 / Fmt::K_PER_BYTE);
    if constexpr (Fmt::STEP_SCALE) r.s = srow[k0 / 32];
  };

  // Per step a wave issues NW VM operations, in this order: 1 W register
  // load, 1 scale byte load with STEP_SCALE, NI X LDS loads. Waiting for NW
  // outstanding means the whole previous step has landed. A load added to
  // the K loop is added here.
  constexpr int NW = 1 + (Fmt::STEP_SCALE ? 1 : 0) + NI;
  constexpr int WAIT_NEXT = waitcnt_vmcnt(NW);
  constexpr int WAIT_0 = waitcnt_vmcnt(0);

  // MFMA over one staged K-step: W from registers, X from tile[buf]
  auto compute = [&](const int buf, const Regs& use) {
    float sc = 1.0f;
    if constexpr (Fmt::STEP_SCALE) sc = e8m0_to_float(use.s);
#pragma unroll
    for (int kk = 0; kk < Fmt::KK; ++kk) {
      const bf16x8_t b = Fmt::cvt8(use.w, kk, sc);
      const int kc = kgrp * Fmt::KK + kk;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        bf16x8_t a = *reinterpret_cast<bf16x8_t*>(
            &tile[buf][lds_row_idx(t * 16 + m_local, kc)]);
        acc[t] = mfma16x16x32(a, b, acc[t]);
      }
    }
  };
  // a step with a successor: prefetch step k0+BK (W into load, X into
  // buf^1), wait until step k0 has landed, compute it. Only called with
  // k0 + BK < k_hi <= K, so the prefetch stays inside the row.
  auto step = [&](const int buf, const int k0, const Regs& use, Regs& load) {
    load_w(load, k0 + BK);
    stage(buf ^ 1, k0 + BK);
    __builtin_amdgcn_s_waitcnt(WAIT_NEXT);  // step k0 landed; next in flight
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();  // raw: no vmcnt drain (counted pipeline)
    compute(buf, use);
    __builtin_amdgcn_s_barrier();  // readers done before tile[buf] is reused
  };
  auto last_step = [&](const int buf, const Regs& use) {
    __builtin_amdgcn_s_waitcnt(WAIT_0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    compute(buf, use);
  };

  // The two W register sets and the two X buffers alternate by name, and
  // the tail is peeled, so the loop body is straight-line code: no register
  // copy on the back edge and no branch around the prefetch, either of
  // which makes the compiler drain vmcnt to 0 before it reads a W register.
  Regs r_a{}, r_b{};
  int k0 = k_lo;
  if (k0 < k_hi) {  // a trailing split can be empty when K/nsplit rounds up
    load_w(r_a, k0);
    stage(0, k0);
    for (; k0 + 2 * BK < k_hi; k0 += 2 * BK) {
      step(0, k0, r_a, r_b);
      step(1, k0 + BK, r_b, r_a);
    }
    if (k0 + BK < k_hi) {
      step(0, k0, r_a, r_b);
      last_step(1, r_b);
    } else {
      last_step(0, r_a);
    }
  }

  // ---- epilogue: C row = token, col = feature; OUT_SCALE in f32 ----
  const int feat = f_base + wave * FEAT_PER_WAVE + MFMA_C_COL(lane);
  float sc = 1.0f;
  if constexpr (Fmt::OUT_SCALE) sc = scale[feat];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int tokn = t * 16 + MFMA_C_ROW(lane, reg);
      if (tokn < N) {
        float c = acc[t][reg];
        if constexpr (Fmt::OUT_SCALE) c *= sc;
        const short v = float_to_bf16_bits(c);
        if constexpr (SPLIT) {
          out_ws[((long)blockIdx.y * N + tokn) * M + feat] = v;
        } else {
          out[(long)tokn * M + feat] = v;
        }
      }
    }
  }
}

template <class Fmt, int NT>
void launch_nt(short* out, short* ws, const short* x, const unsigned char* w,
               const typename Fmt::scale_t* scale, int M, int K, int N,
               long xs, int nsplit, int k_per_split, hipStream_t stream) {
  dim3 grid(M / (NWAVES * FEAT_PER_WAVE), nsplit);
  if (nsplit > 1) {
    hipLaunchKernelGGL((skinny_gemm_wq_kernel<Fmt, NT, true>), grid,
                       dim3(256), 0, stream, out, ws, x, w, scale, M, K, N,
                       xs, k_per_split);
  } else {
    hipLaunchKernelGGL((skinny_gemm_wq_kernel<Fmt, NT, false>), grid,
                       dim3(256), 0, stream, out, ws, x, w, scale, M, K, N,
                       xs, k_per_split);
  }
}

template <class Fmt>
hipError_t skinny_gemm_wq(void* out, void* workspace, const void* x,
                          const void* qweight, const void* scale, int M,
                          int K, int N, long x_row_stride,
                          hipStream_t stream) {
  constexpr int BK = Fmt::BK;
  if (M <= 0 || M % 64 != 0 || K <= 0 || K % BK != 0 || N < 1 ||
      N > Fmt::MAX_N)
    return hipErrorInvalidValue;
  // 16-byte global_load_lds sources / W register loads (a W row is a
  // multiple of 64 bytes, so every row start keeps the base alignment)
  if (x_row_stride % 8 != 0 || ((uintptr_t)x & 15) != 0 ||
      ((uintptr_t)qweight & 15) != 0)
    return hipErrorInvalidValue;
  const int nsplit = ks_skinny_nsplit(M, K, BK);
  if (nsplit > 1 && workspace == nullptr) return hipErrorInvalidValue;
  const int k_per_split = ((K / nsplit + BK - 1) / BK) * BK;
  const int NT = (N + 15) / 16;
  short* ws = (short*)workspace;
#define CASE(nt)                                                          \
  launch_nt<Fmt, nt>((short*)out, ws, (const short*)x,                    \
                     (const unsigned char*)qweight,                       \
                     (const typename Fmt::scale_t*)scale, M, K, N,        \
                     x_row_stride, nsplit, k_per_split, stream)
  switch (NT) {
    case 1: CASE(1); break;
    case 2: CASE(2); break;
    case 3: CASE(3); break;
    case 4: CASE(4); break;
    case 5: CASE(5); break;
    case 6: CASE(6); break;
    case 7: CASE(8); break;
    case 8: CASE(8); break;
    default:  // N <= MAX_N was checked above
      if constexpr (Fmt::MAX_N > 128) {
        if (NT <= 12) CASE(12);
        else CASE(16);
      }
      break;
  }
#undef CASE
  HIP_CHECK_KERNEL();
  if (nsplit > 1)
    return ks_reduce_bf16_partials((short*)out, ws, (long)N * M, nsplit,
                                   stream);
  return hipSuccess;
}

// 16 fp8 bytes in, 2 x 16 B bf16 out per lane-iteration
__global__ __launch_bounds__(256) void dequant_fp8_rows_kernel(
    short* __restrict__ out, const unsigned char* __restrict__ q,
    const float* __restrict__ scale, const long nchunks, const int K) {
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < nchunks;
       c += (long)gridDim.x * blockDim.x) {
    const long e = c * 16;
    const float sc = scale[e / K];  // K % 16 == 0: a chunk stays in one row
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(q + e);
    short8_t o[2];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const float2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[d], false);
      const float2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[d], true);
      o[d >> 1][(d & 1) * 4 + 0] = float_to_bf16_bits(lo[0] * sc);
      o[d >> 1][(d & 1) * 4 + 1] = float_to_bf16_bits(lo[1] * sc);
      o[d >> 1][(d & 1) * 4 + 2] = float_to_bf16_bits(hi[0] * sc);
      o[d >> 1][(d & 1) * 4 + 3] = float_to_bf16_bits(hi[1] * sc);
    }
    *reinterpret_cast<short8_t*>(out + e) = o[0];
    *reinterpret_cast<short8_t*>(out + e + 8) = o[1];
  }
}

// odd K (not a multiple of 16): one element per lane-iteration
__global__ __launch_bounds__(256) void dequant_fp8_rows_scalar_kernel(
    short* __restrict__ out, const unsigned char* __restrict__ q,
    const float* __restrict__ scale, const long n, const int K) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n;
       e += (long)gridDim.x * blockDim.x) {
    const float2_t f = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[e], false);
    out[e] = float_to_bf16_bits(f[0] * scale[e / K]);
  }
}

// one MX block per lane-iteration: 16 B of codes + 1 scale byte in,
// 4 x 16 B bf16 out. The same convert as the GEMM, so the two agree.
__global__ __launch_bounds__(256) void dequant_mxfp4_rows_kernel(
    short* __restrict__ out, const unsigned char* __restrict__ q,
    const unsigned char* __restrict__ scale, const long nblocks) {
  for (long b = blockIdx.x * (long)blockDim.x + threadIdx.x; b < nblocks;
       b += (long)gridDim.x * blockDim.x) {
    // rows are contiguous and K % 32 == 0: block b of the flat array is
    // bytes [16b, 16b+16) of q and scale byte b
    const float sc = e8m0_to_float(scale[b]);
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(q + b * 16);
#pragma unroll
    for (int d = 0; d < 4; ++d)
      *reinterpret_cast<bf16x8_t*>(out + b * 32 + d * 8) =
          Mxfp4::cvt8(v, d, sc);
  }
}

}  // namespace

extern "C" hipError_t ks_skinny_gemm_w8(void* out, void* workspace,
                                        const void* x, const void* qweight,
                                        const void* scale, int M, int K,
                                        int N, long x_row_stride,
                                        hipStream_t stream) {
  return skinny_gemm_wq<Fp8>(out, workspace, x, qweight, scale, M, K, N,
                             x_row_stride, stream);
}

extern "C" hipError_t ks_skinny_gemm_w4(void* out, void* workspace,
                                        const void* x, const void* qweight,
                                        const void* scale, int M, int K,
                                        int N, long x_row_stride,
                                        hipStream_t stream) {
  return skinny_gemm_wq<Mxfp4>(out, workspace, x, qweight, scale, M, K, N,
                               x_row_stride, stream);
}

extern "C" hipError_t ks_dequant_fp8_rows(void* out, const void* qweight,
                                          const void* scale, long M, int K,
                                          hipStream_t stream) {
  if (M <= 0 || K <= 0) return hipErrorInvalidValue;
  const long n = M * (long)K;
  if (K % 16 == 0 && ((uintptr_t)qweight & 15) == 0 &&
      ((uintptr_t)out & 15) == 0) {
    const long nchunks = n / 16;
    const int blocks = (int)min((nchunks + 255) / 256, (long)4096);
    hipLaunchKernelGGL(dequant_fp8_rows_kernel, dim3(blocks), dim3(256), 0,
                       stream, (short*)out, (const unsigned char*)qweight,
                       (const float*)scale, nchunks, K);
  } else {
    const int blocks = (int)min((n + 255) / 256, (long)4096);
    hipLaunchKernelGGL(dequant_fp8_rows_scalar_kernel, dim3(blocks),
                       dim3(256), 0, stream, (short*)out,
                       (const unsigned char*)qweight, (const float*)scale, n,
                       K);
  }
  HIP_CHECK_KERNEL();
  return hipSuccess;
}

extern "C" hipError_t ks_dequant_mxfp4_rows(void* out, const void* qweight,
                                            const void* scale, long M, int K,
                                            hipStream_t stream) {
  if (M <= 0 || K <= 0 || K % 32 != 0) return hipErrorInvalidValue;
  if (((uintptr_t)qweight & 15) != 0 || ((uintptr_t)out & 15) != 0)
    return hipErrorInvalidValue;
  const long nblocks = M * (long)(K / 32);
  const int blocks = (int)min((nblocks + 255) / 256, (long)4096);
  hipLaunchKernelGGL(dequant_mxfp4_rows_kernel, dim3(blocks), dim3(256), 0,
                     stream, (short*)out, (const unsigned char*)qweight,
                     (const unsigned char*)scale, nblocks);
  HIP_CHECK_KERNEL();
  return hipSuccess;
}
