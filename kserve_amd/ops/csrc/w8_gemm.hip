// Weight-only fp8 (OCP E4M3, W8A16) decode GEMM and row dequantizer.
//
//   ks_skinny_gemm_w8:   out[N][M] bf16 = (x[N][K] bf16 @ q[M][K]^T fp8) * scale[M]
//   ks_dequant_fp8_rows: out[M][K] bf16 = bf16_rne(float(q[M][K]) * scale[M])
//
// The GEMM keeps skinny_gemm.hip's structure (4 waves x 16 features, X tile
// shared through LDS with pre-swizzled global_load_lds sources, counted-vmcnt
// double buffer, NT template over token tiles, K-split into disjoint bf16
// partials + a reduce kernel). What changes is the W side: every W row is
// read by exactly one wave, so W never goes through LDS. Each lane loads 16
// consecutive K bytes of its feature row straight into registers (one
// global_load_dwordx4 per BK=64 step, prefetched one step ahead like the X
// tile), converts them in registers with cvt_scalef32_pk_bf16_fp8 (exact:
// E4M3 fits bf16's mantissa) and feeds v_mfma_f32_16x16x32_bf16. The
// per-channel scale multiplies the f32 accumulator in the epilogue, after
// the K reduction (before the bf16 partial is written in the split-K
// variant), so the only approximation is the one-time weight rounding.
//
// K order: lane (kgrp = lane >> 4) holds W bytes K = k0 + kgrp*16 + [0,16);
// MFMA kk in {0,1} consumes bytes kk*8..kk*8+7, i.e. X chunk (8 bf16)
// kc = kgrp*2 + kk. MFMA only needs A and B to agree on which K sits in
// which (lane, j) slot, so the X fragment simply reads that chunk.
#include "common.h"
#include "mfma_layouts.h"

namespace {

constexpr int BK = 64;  // K per stage step
constexpr int FEAT_PER_WAVE = 16;
constexpr int NWAVES = 4;  // 64 features per workgroup

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

// X tile swizzle. chunk = 8 bf16 = 16 B, row = 8 chunks = 128 B. One
// ds_read_b128 serves lanes of two adjacent kgrp values together (e.g.
// lanes 0-3,12-15 with 20-27), which here read chunks kc and kc^2; the
// skinny_gemm swizzle kc ^ (row & 7) would put both on the same bank
// parity (2-way conflict). Folding bit 1 of kc into bit 0 first makes the
// two chunk positions differ in parity, so the 16 lanes of a group cover
// 16 distinct 4-bank slots. chunk_perm is an involution (bit 1 is kept).
__device__ __forceinline__ int chunk_perm(int kc) {
  return kc ^ ((kc >> 1) & 1);
}
__device__ __forceinline__ int lds_row_idx(int row, int kc) {
  return (row * (BK / 8) + (chunk_perm(kc) ^ (row & 7))) * 8;  // shorts
}

// 8 fp8 bytes (two dwords) -> 8 bf16, element order = byte order
__device__ __forceinline__ bf16x8_t cvt8(unsigned int lo, unsigned int hi) {
  const bf16x2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
  const bf16x2_t p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
  const bf16x2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
  const bf16x2_t p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
  return bf16x8_t{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

template <int NT, bool SPLIT>
__global__ __launch_bounds__(256) void skinny_gemm_w8_kernel(
    short* __restrict__ out,      // [N][M] bf16 (!SPLIT)
    short* __restrict__ out_ws,   // [nsplit][N][M] bf16 partials (SPLIT)
    const short* __restrict__ x,  // [N][K] row stride xs
    const unsigned char* __restrict__ w,  // [M][K] e4m3 bytes
    const float* __restrict__ scale,      // [M]
    const int M, const int K, const int N, const long xs,
    const int k_per_split) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int f_base = blockIdx.x * (NWAVES * FEAT_PER_WAVE);
  const int k_lo = blockIdx.y * k_per_split;
  const int k_hi = min(K, k_lo + k_per_split);

  // LDS: double-buffered X tile [NT*16][BK], swizzled, + one 1 KB scratch
  // slot for stage-count padding
  constexpr int X_CHUNKS = NT * 16 * (BK / 8);  // 16B chunks
  constexpr int NINSTR = X_CHUNKS / 64;         // wg-wide 1 KB instrs
  constexpr int NI = (NINSTR + NWAVES - 1) / NWAVES;  // per-wave, padded
  constexpr int TILE_SHORTS = NT * 16 * BK;
  __shared__ short tile[2][TILE_SHORTS];
  __shared__ short scratch[512];  // dump target for padding instrs

  f32x4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int m_local = lane & 15;
  const int kgrp = lane >> 4;
  // this lane's W stream: its feature row, 16 bytes per K-step
  const unsigned char* wrow =
      w + (long)(f_base + wave * FEAT_PER_WAVE + m_local) * K + kgrp * 16;

  // stage the X BK-slice at k-offset k0 into buf; every wave issues exactly
  // NI instructions so the counted s_waitcnt below is uniform
  auto stage = [&](int buf, int k0) {
#pragma unroll
    for (int ii = 0; ii < NI; ++ii) {
      const int i = wave + ii * NWAVES;
      const int g = i * 64 + lane;
      const short* src;
      short* dst;
      if (i < NINSTR) {
        dst = &tile[buf][i * 64 * 8];
        int row = g >> 3;  // token row
        const int kc_src = chunk_perm((g & 7) ^ (row & 7));
        if (row >= N) row = N - 1;  // clamp padded token rows
        src = x + (long)row * xs + (kc_src << 3) + k0;
      } else {  // padding instr keeps per-wave vmcnt uniform
        dst = scratch;
        src = x;
      }
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const unsigned int*>(src),
          reinterpret_cast<unsigned int*>(dst), 16, 0, 0);
    }
  };

  // s_waitcnt imm: vmcnt==n, ignore lgkm/exp (gfx9 encoding:
  // vmcnt[3:0]|vmcnt[5:4]<<14, expcnt[6:4], lgkmcnt[11:8]). Per step a wave
  // issues {1 W register load, NI X LDS loads} in that order; waiting for
  // NI+1 outstanding means the whole previous step has landed.
  constexpr int NW = NI + 1;
  constexpr int WAIT_NEXT =
      (0xF << 8) | (0x7 << 4) | (NW & 0xF) | (((NW >> 4) & 0x3) << 14);
  constexpr int WAIT_0 = (0xF << 8) | (0x7 << 4);

  // MFMA over one staged K-step: W from registers, X from tile[buf]
  auto compute = [&](const int buf, const u32x4_t& w_use) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const bf16x8_t b = cvt8(w_use[kk * 2], w_use[kk * 2 + 1]);
      const int kc = kgrp * 2 + kk;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        bf16x8_t a = *reinterpret_cast<bf16x8_t*>(
            &tile[buf][lds_row_idx(t * 16 + m_local, kc)]);
        acc[t] = mfma16x16x32(a, b, acc[t]);
      }
    }
  };
  // a step with a successor: prefetch step k0+BK (W into w_load, X into
  // buf^1), wait until step k0 has landed, compute it
  auto step = [&](const int buf, const int k0, const u32x4_t& w_use,
                  u32x4_t& w_load) {
    w_load = *reinterpret_cast<const u32x4_t*>(wrow + k0 + BK);
    stage(buf ^ 1, k0 + BK);
    __builtin_amdgcn_s_waitcnt(WAIT_NEXT);  // step k0 landed; next in flight
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();  // raw: no vmcnt drain (counted pipeline)
    compute(buf, w_use);
    __builtin_amdgcn_s_barrier();  // readers done before tile[buf] is reused
  };
  auto last_step = [&](const int buf, const u32x4_t& w_use) {
    __builtin_amdgcn_s_waitcnt(WAIT_0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    compute(buf, w_use);
  };

  // The two W registers and the two X buffers alternate by name, and the
  // tail is peeled, so the loop body is straight-line code: no register
  // copy on the back edge and no branch around the prefetch, either of
  // which makes the compiler drain vmcnt to 0 before it reads a W register.
  u32x4_t w_a = u32x4_t{0u, 0u, 0u, 0u};
  u32x4_t w_b = u32x4_t{0u, 0u, 0u, 0u};
  int k0 = k_lo;
  if (k0 < k_hi) {  // a trailing split can be empty when K/nsplit rounds up
    w_a = *reinterpret_cast<const u32x4_t*>(wrow + k0);
    stage(0, k0);
    for (; k0 + 2 * BK < k_hi; k0 += 2 * BK) {
      step(0, k0, w_a, w_b);
      step(1, k0 + BK, w_b, w_a);
    }
    if (k0 + BK < k_hi) {
      step(0, k0, w_a, w_b);
      last_step(1, w_b);
    } else {
      last_step(0, w_a);
    }
  }

  // ---- epilogue: C row = token, col = feature; scale in f32 ----
  const int feat = f_base + wave * FEAT_PER_WAVE + MFMA_C_COL(lane);
  const float sc = scale[feat];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int tokn = t * 16 + MFMA_C_ROW(lane, reg);
      if (tokn < N) {
        const short v = float_to_bf16_bits(acc[t][reg] * sc);
        if constexpr (SPLIT) {
          out_ws[((long)blockIdx.y * N + tokn) * M + feat] = v;
        } else {
          out[(long)tokn * M + feat] = v;
        }
      }
    }
  }
}

// sum bf16 partials (f32 accumulate) and store bf16
__global__ void reduce_ws_w8_kernel(short* __restrict__ out,
                                    const short* __restrict__ ws,
                                    const long nm, const int nsplit) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nm;
       i += (long)gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int s = 0; s < nsplit; ++s)
      acc += bf16_bits_to_float(ws[s * nm + i]);
    out[i] = float_to_bf16_bits(acc);
  }
}

template <int NT>
void launch_nt(short* out, short* ws, const short* x, const unsigned char* w,
               const float* scale, int M, int K, int N, long xs, int nsplit,
               int k_per_split, hipStream_t stream) {
  dim3 grid(M / (NWAVES * FEAT_PER_WAVE), nsplit);
  if (nsplit > 1) {
    hipLaunchKernelGGL((skinny_gemm_w8_kernel<NT, true>), grid, dim3(256), 0,
                       stream, out, ws, x, w, scale, M, K, N, xs,
                       k_per_split);
  } else {
    hipLaunchKernelGGL((skinny_gemm_w8_kernel<NT, false>), grid, dim3(256), 0,
                       stream, out, ws, x, w, scale, M, K, N, xs,
                       k_per_split);
  }
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

}  // namespace

// the K-split both the launcher and the binding (workspace size) use
extern "C" int ks_skinny_gemm_w8_nsplit(int M, int K) {
  const int feat_wgs = M / 64;
  int nsplit = 1;
  while (feat_wgs * nsplit < 768 && nsplit < 8 && (K / (nsplit * 2)) >= BK)
    nsplit *= 2;
  return nsplit;
}

extern "C" hipError_t ks_skinny_gemm_w8(void* out, void* workspace,
                                        const void* x, const void* qweight,
                                        const void* scale, int M, int K,
                                        int N, long x_row_stride,
                                        hipStream_t stream) {
  if (M <= 0 || M % 64 != 0 || K <= 0 || K % BK != 0 || N < 1 || N > 256)
    return hipErrorInvalidValue;
  // 16-byte global_load_lds sources / W register loads
  if (x_row_stride % 8 != 0 || ((uintptr_t)x & 15) != 0 ||
      ((uintptr_t)qweight & 15) != 0)
    return hipErrorInvalidValue;
  // fill the chip: aim for >= 768 workgroups via K-splits
  const int nsplit = ks_skinny_gemm_w8_nsplit(M, K);
  if (nsplit > 1 && workspace == nullptr) return hipErrorInvalidValue;
  const int k_per_split = ((K / nsplit + BK - 1) / BK) * BK;
  const int NT = (N + 15) / 16;
  short* ws = (short*)workspace;
  const short* xp = (const short*)x;
  const unsigned char* wp = (const unsigned char*)qweight;
  const float* sp = (const float*)scale;
#define CASE(nt)                                                             \
  launch_nt<nt>((short*)out, ws, xp, wp, sp, M, K, N, x_row_stride, nsplit, \
                k_per_split, stream)
  switch (NT) {
    case 1: CASE(1); break;
    case 2: CASE(2); break;
    case 3: CASE(3); break;
    case 4: CASE(4); break;
    case 5: CASE(5); break;
    case 6: CASE(6); break;
    case 7: CASE(8); break;
    case 8: CASE(8); break;
    default:
      if (NT <= 12) CASE(12);
      else CASE(16);
      break;
  }
#undef CASE
  HIP_CHECK_KERNEL();
  if (nsplit > 1) {
    const long nm = (long)N * M;
    hipLaunchKernelGGL(reduce_ws_w8_kernel, dim3(2048), dim3(256), 0, stream,
                       (short*)out, ws, nm, nsplit);
    HIP_CHECK_KERNEL();
  }
  return hipSuccess;
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
