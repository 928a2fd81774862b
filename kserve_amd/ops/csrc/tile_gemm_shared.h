// What the 128 x 128 x 64 MFMA tile GEMMs (moe_prefill.hip, grouped experts;
// wq_tile_gemm.hip, dense quantized projections) share, defined once: the LDS
// swizzles of the X and W tiles and the weight formats as a W tile holds
// them. The converts themselves are wq_formats.h's.
#pragma once

#include "common.h"
#include "mfma_layouts.h"
#include "wq_formats.h"

namespace {

// LDS swizzle on a byte offset inside a [128][64] bf16 tile (gemm8.hip
// SW = 2): the 16 B granule index, bits 4..7, is XORed with (row >> 1) & 15.
// An involution; the 16 lanes of a fragment read cover all 64 banks once.
__device__ __forceinline__ int swz(int byte_off) {
  return byte_off ^ (((byte_off >> 8) & 15) << 4);
}

// ---- weight formats of a W tile ----
//
// ROW_BYTES    bytes of one W row in a K step (BK = 64 elements)
// STEP_SCALE   one E8M0 byte per W row and 32 K, applied in the convert
// OUT_SCALE    one f32 scale per W row, applied to the accumulator
// frag         the 8 bf16 of one MFMA from a lane's LDS read (raw_t)
struct PfBf16 {
  static constexpr int ROW_BYTES = 128;
  static constexpr bool STEP_SCALE = false;
  static constexpr bool OUT_SCALE = false;
  using scale_t = float;  // unused
  using raw_t = bf16x8_t;
  static __device__ __forceinline__ bf16x8_t frag(const raw_t& r, float) {
    return r;
  }
};

struct PfFp8 {
  static constexpr int ROW_BYTES = 64;
  static constexpr bool STEP_SCALE = false;
  static constexpr bool OUT_SCALE = true;
  using scale_t = float;
  typedef unsigned int raw_t __attribute__((ext_vector_type(2)));
  static __device__ __forceinline__ bf16x8_t frag(const raw_t& r, float) {
    return Fp8::cvt8(r[0], r[1]);
  }
};

struct PfMxfp4 {
  static constexpr int ROW_BYTES = 32;
  static constexpr bool STEP_SCALE = true;
  static constexpr bool OUT_SCALE = false;
  using scale_t = unsigned char;
  using raw_t = unsigned int;
  static __device__ __forceinline__ bf16x8_t frag(const raw_t& r, float sc) {
    return Mxfp4::cvt8(r, sc);
  }
};

// Swizzle of the W tile, [128][ROW_BYTES]: bf16 rows are the X tile's. A
// quantized row has ROW_BYTES / 16 granules (bits 4.. of the offset) and 256
// bytes, one turn of the 64 banks, hold 256 / ROW_BYTES rows; the granule
// index is XORed with the row bits from offset bit 8 up, the rows that would
// land on the same banks. An involution, the key of a fragment's 16 rows
// depends on the lane alone (16 rows are 1024 or 512 bytes, above the key).
template <int ROW_BYTES>
__device__ __forceinline__ int wswz(int byte_off) {
  if constexpr (ROW_BYTES == 128) return swz(byte_off);
  return byte_off ^ (((byte_off >> 8) & (ROW_BYTES / 16 - 1)) << 4);
}

}  // namespace
