// The weight-only quantized formats (kserve_amd/ops/quant.py) as the kernels
// see them: what wq_gemm.hip (dense decode GEMM), moe.hip and moe_prefill.hip
// (routed expert GEMMs) do differently per format. Everything here is exact: E4M3 and
// E2M1 * 2^e both fit bf16, so the only approximation is the one-time
// rounding of the weights.
//
// Stored MXFP4: byte i of a row holds element 2i in bits 3:0 and element
// 2i+1 in bits 7:4; one E8M0 scale byte per 32 elements of a row.
#pragma once
#include "common.h"
#include "mfma_layouts.h"

namespace {

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

// ---- the two formats ----
//
// BK           K per stage step; an X tile row is BK/8 chunks of 8 bf16
// KK           MFMAs per step per token tile
// K_PER_BYTE   K elements in one W byte
// scale_t      element type of the scale array
// STEP_SCALE   a lane loads one scale byte per step (row of K/32 bytes)
//              and the convert applies it
// OUT_SCALE    the epilogue multiplies by scale[feature]
// MAX_N        most tokens; wq_gemm.hip's NT switch stops there
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
    return cvt8(w[kk * 2], w[kk * 2 + 1]);
  }
  // the same from the two dwords themselves (moe_prefill.hip reads 8 B of a
  // W row from LDS per MFMA)
  static __device__ __forceinline__ bf16x8_t cvt8(const unsigned int lo,
                                                  const unsigned int hi) {
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
    return cvt8(w[kk], sc);
  }
  // the same from the dword itself (moe_prefill.hip reads 4 B of a W row
  // from LDS per MFMA)
  static __device__ __forceinline__ bf16x8_t cvt8(unsigned int v,
                                                  const float sc) {
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

// what one K-step of W occupies in a lane's registers (wq_gemm.hip)
template <bool STEP_SCALE>
struct WRegs {
  u32x4_t w;
};
template <>
struct WRegs<true> {
  u32x4_t w;
  unsigned int s;
};

}  // namespace
