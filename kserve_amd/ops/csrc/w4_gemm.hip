// Weight-only MXFP4 (OCP E2M1 + E8M0 block scale, W4A16) decode GEMM and
// row dequantizer.
//
//   ks_skinny_gemm_w4:     out[N][M] bf16 = x[N][K] bf16 @ dequant(q, s)[M][K]^T
//   ks_dequant_mxfp4_rows: out[M][K] bf16 = e2m1(q[M][K/2]) * 2^(s[M][K/32]-127)
//
// Stored format (kserve_amd/ops/quant.py): byte i of a row holds element 2i
// in bits 3:0 and element 2i+1 in bits 7:4; one E8M0 scale byte per 32
// consecutive elements of a row.
//
// The GEMM keeps w8_gemm.hip's structure (4 waves x 16 features, X tile
// shared through LDS with pre-swizzled global_load_lds sources, W straight
// from global into registers, counted-vmcnt double buffer with raw
// s_barrier, NT template over token tiles, K-split into disjoint bf16
// partials + a reduce kernel). What changes is the K geometry: a lane still
// loads 16 B of its feature row per step (the fp8 kernel lost byte rate by
// halving the bytes in flight per load, profiles/w8_gemm.md), which is now
// 32 consecutive K, so BK = 128 and a step is four 16x16x32 MFMAs per token
// tile. Those 16 B are exactly one MX block: the lane loads one scale byte
// per step and applies it inside cvt_scalef32_pk_bf16_fp4, which is exact
// (the scale is a power of two), so there is no scale in the epilogue.
//
// K order: lane (kgrp = lane >> 4) holds W elements K = k0 + kgrp*32 +
// [0,32); MFMA kk in {0..3} consumes dword kk of the 16 B, i.e. elements
// kk*8..kk*8+7, i.e. X chunk (8 bf16) kc = kgrp*4 + kk. MFMA only needs A
// and B to agree on which K sits in which (lane, j) slot, so the X fragment
// simply reads that chunk.
#include "common.h"
#include "mfma_layouts.h"

namespace {

constexpr int BK = 128;  // K per stage step
constexpr int FEAT_PER_WAVE = 16;
constexpr int NWAVES = 4;  // 64 features per workgroup
constexpr int MAX_N = 128;

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

// The hardware convert reads the byte's bits 3:0 as the first element of
// the pair, which is the stored order. Were it the other way round, the
// fix is in registers (swap the nibbles of every byte), not in the format.
constexpr bool SWAP_NIBBLES = false;

// X tile swizzle. chunk = 8 bf16 = 16 B, row = 16 chunks = 256 B = one full
// LDS bank row, so the slot (4 banks) of a chunk is its position in the row.
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
// involution (bit 2 is kept). The fp8 kernel's perm (bit 1 into bit 0) is
// the same argument for its 8-chunk rows and does not separate these.
__device__ __forceinline__ int chunk_perm(int kc) {
  return kc ^ ((kc & 4) << 1);
}
__device__ __forceinline__ int lds_row_idx(int row, int kc) {
  return (row * (BK / 8) + (chunk_perm(kc) ^ (row & 15))) * 8;  // shorts
}

// E8M0 code -> the f32 with that biased exponent (2^(c-127))
__device__ __forceinline__ float e8m0_to_float(unsigned int c) {
  return __uint_as_float(c << 23);
}

// 8 fp4 nibbles (one dword) -> 8 bf16 times the block scale, element order
// = nibble order
__device__ __forceinline__ bf16x8_t cvt8(unsigned int v, const float sc) {
  if constexpr (SWAP_NIBBLES)
    v = ((v & 0x0f0f0f0fu) << 4) | ((v >> 4) & 0x0f0f0f0fu);
  const bf16x2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 0);
  const bf16x2_t p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 1);
  const bf16x2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 2);
  const bf16x2_t p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, 3);
  return bf16x8_t{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

template <int NT, bool SPLIT>
__global__ __launch_bounds__(256) void skinny_gemm_w4_kernel(
    short* __restrict__ out,      // [N][M] bf16 (!SPLIT)
    short* __restrict__ out_ws,   // [nsplit][N][M] bf16 partials (SPLIT)
    const short* __restrict__ x,  // [N][K] row stride xs
    const unsigned char* __restrict__ w,      // [M][K/2] packed e2m1
    const unsigned char* __restrict__ scale,  // [M][K/32] e8m0
    const int M, const int K, const int N, const long xs,
    const int k_per_split) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int f_base = blockIdx.x * (NWAVES * FEAT_PER_WAVE);
  const int k_lo = blockIdx.y * k_per_split;
  const int k_hi = min(K, k_lo + k_per_split);

  // LDS: double-buffered X tile [NT*16][BK], swizzled. A tile is NT*4
  // wg-wide 1 KB instructions, i.e. exactly NT per wave: no padding
  // instruction is needed to keep the per-wave vmcnt uniform.
  constexpr int NI = NT;  // glds instructions per wave per step
  constexpr int TILE_SHORTS = NT * 16 * BK;
  __shared__ short tile[2][TILE_SHORTS];

  f32x4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int m_local = lane & 15;
  const int kgrp = lane >> 4;
  // this lane's W stream: its feature row, 16 bytes (32 K) per K-step,
  // and the scale byte of that block
  const long frow = f_base + wave * FEAT_PER_WAVE + m_local;
  const unsigned char* wrow = w + frow * (K / 2) + kgrp * 16;
  const unsigned char* srow = scale + frow * (K / 32) + kgrp;

  // stage the X BK-slice at k-offset k0 into buf
  auto stage = [&](int buf, int k0) {
#pragma unroll
    for (int ii = 0; ii < NI; ++ii) {
      const int i = wave + ii * NWAVES;
      const int g = i * 64 + lane;
      short* dst = &tile[buf][i * 64 * 8];
      int row = g >> 4;  // token row
      const int kc_src = chunk_perm((g & 15) ^ (row & 15));
      if (row >= N) row = N - 1;  // clamp padded token rows
      const short* src = x + (long)row * xs + (kc_src << 3) + k0;
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const unsigned int*>(src),
          reinterpret_cast<unsigned int*>(dst), 16, 0, 0);
    }
  };

  // s_waitcnt imm: vmcnt==n, ignore lgkm/exp (gfx9 encoding:
  // vmcnt[3:0]|vmcnt[5:4]<<14, expcnt[6:4], lgkmcnt[11:8]). Per step a wave
  // issues {1 W register load, 1 scale byte load, NI X LDS loads} in that
  // order; waiting for NI+2 outstanding means the whole previous step has
  // landed.
  constexpr int NW = NI + 2;
  constexpr int WAIT_NEXT =
      (0xF << 8) | (0x7 << 4) | (NW & 0xF) | (((NW >> 4) & 0x3) << 14);
  constexpr int WAIT_0 = (0xF << 8) | (0x7 << 4);

  // MFMA over one staged K-step: W from registers, X from tile[buf]
  auto compute = [&](const int buf, const u32x4_t& w_use,
                     const unsigned int s_use) {
    const float sc = e8m0_to_float(s_use);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const bf16x8_t b = cvt8(w_use[kk], sc);
      const int kc = kgrp * 4 + kk;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        bf16x8_t a = *reinterpret_cast<bf16x8_t*>(
            &tile[buf][lds_row_idx(t * 16 + m_local, kc)]);
        acc[t] = mfma16x16x32(a, b, acc[t]);
      }
    }
  };
  // a step with a successor: prefetch step k0+BK (W and its scale into
  // w_load/s_load, X into buf^1), wait until step k0 has landed, compute
  // it. Only called with k0 + BK < k_hi <= K, so the prefetch stays inside
  // the row.
  auto step = [&](const int buf, const int k0, const u32x4_t& w_use,
                  const unsigned int s_use, u32x4_t& w_load,
                  unsigned int& s_load) {
    w_load = *reinterpret_cast<const u32x4_t*>(wrow + (k0 + BK) / 2);
    s_load = srow[(k0 + BK) / 32];
    stage(buf ^ 1, k0 + BK);
    __builtin_amdgcn_s_waitcnt(WAIT_NEXT);  // step k0 landed; next in flight
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();  // raw: no vmcnt drain (counted pipeline)
    compute(buf, w_use, s_use);
    __builtin_amdgcn_s_barrier();  // readers done before tile[buf] is reused
  };
  auto last_step = [&](const int buf, const u32x4_t& w_use,
                       const unsigned int s_use) {
    __builtin_amdgcn_s_waitcnt(WAIT_0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    compute(buf, w_use, s_use);
  };

  // The two W/scale register sets and the two X buffers alternate by name,
  // and the tail is peeled, so the loop body is straight-line code: no
  // register copy on the back edge and no branch around the prefetch,
  // either of which makes the compiler drain vmcnt to 0 before it reads a
  // W register.
  u32x4_t w_a = u32x4_t{0u, 0u, 0u, 0u};
  u32x4_t w_b = u32x4_t{0u, 0u, 0u, 0u};
  unsigned int s_a = 0u, s_b = 0u;
  int k0 = k_lo;
  if (k0 < k_hi) {  // a trailing split can be empty when K/nsplit rounds up
    w_a = *reinterpret_cast<const u32x4_t*>(wrow + k0 / 2);
    s_a = srow[k0 / 32];
    stage(0, k0);
    for (; k0 + 2 * BK < k_hi; k0 += 2 * BK) {
      step(0, k0, w_a, s_a, w_b, s_b);
      step(1, k0 + BK, w_b, s_b, w_a, s_a);
    }
    if (k0 + BK < k_hi) {
      step(0, k0, w_a, s_a, w_b, s_b);
      last_step(1, w_b, s_b);
    } else {
      last_step(0, w_a, s_a);
    }
  }

  // ---- epilogue: C row = token, col = feature ----
  const int feat = f_base + wave * FEAT_PER_WAVE + MFMA_C_COL(lane);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int tokn = t * 16 + MFMA_C_ROW(lane, reg);
      if (tokn < N) {
        const short v = float_to_bf16_bits(acc[t][reg]);
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
__global__ void reduce_ws_w4_kernel(short* __restrict__ out,
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
               const unsigned char* scale, int M, int K, int N, long xs,
               int nsplit, int k_per_split, hipStream_t stream) {
  dim3 grid(M / (NWAVES * FEAT_PER_WAVE), nsplit);
  if (nsplit > 1) {
    hipLaunchKernelGGL((skinny_gemm_w4_kernel<NT, true>), grid, dim3(256), 0,
                       stream, out, ws, x, w, scale, M, K, N, xs,
                       k_per_split);
  } else {
    hipLaunchKernelGGL((skinny_gemm_w4_kernel<NT, false>), grid, dim3(256), 0,
                       stream, out, ws, x, w, scale, M, K, N, xs,
                       k_per_split);
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
      *reinterpret_cast<bf16x8_t*>(out + b * 32 + d * 8) = cvt8(v[d], sc);
  }
}

}  // namespace

// the K-split both the launcher and the binding (workspace size) use
extern "C" int ks_skinny_gemm_w4_nsplit(int M, int K) {
  const int feat_wgs = M / 64;
  int nsplit = 1;
  while (feat_wgs * nsplit < 768 && nsplit < 8 && (K / (nsplit * 2)) >= BK)
    nsplit *= 2;
  return nsplit;
}

extern "C" hipError_t ks_skinny_gemm_w4(void* out, void* workspace,
                                        const void* x, const void* qweight,
                                        const void* scale, int M, int K,
                                        int N, long x_row_stride,
                                        hipStream_t stream) {
  if (M <= 0 || M % 64 != 0 || K <= 0 || K % BK != 0 || N < 1 || N > MAX_N)
    return hipErrorInvalidValue;
  // 16-byte global_load_lds sources / W register loads (a W row is K/2
  // bytes, a multiple of 64, so every row start keeps the base alignment)
  if (x_row_stride % 8 != 0 || ((uintptr_t)x & 15) != 0 ||
      ((uintptr_t)qweight & 15) != 0)
    return hipErrorInvalidValue;
  // fill the chip: aim for >= 768 workgroups via K-splits
  const int nsplit = ks_skinny_gemm_w4_nsplit(M, K);
  if (nsplit > 1 && workspace == nullptr) return hipErrorInvalidValue;
  const int k_per_split = ((K / nsplit + BK - 1) / BK) * BK;
  const int NT = (N + 15) / 16;
  short* ws = (short*)workspace;
  const short* xp = (const short*)x;
  const unsigned char* wp = (const unsigned char*)qweight;
  const unsigned char* sp = (const unsigned char*)scale;
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
    default: CASE(8); break;  // 7, 8 (N <= 128 was checked above)
  }
#undef CASE
  HIP_CHECK_KERNEL();
  if (nsplit > 1) {
    const long nm = (long)N * M;
    hipLaunchKernelGGL(reduce_ws_w4_kernel, dim3(2048), dim3(256), 0, stream,
                       (short*)out, ws, nm, nsplit);
    HIP_CHECK_KERNEL();
  }
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
