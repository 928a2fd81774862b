// What the skinny decode GEMMs (skinny_gemm.hip, wq_gemm.hip) share, defined
// once: the K-split policy, the reduce over bf16 partials (both in
// skinny_gemm.hip) and the counted-wait immediate (skinny_gemm_kernel's body
// still spells its two immediates out).
#pragma once

#include <hip/hip_runtime.h>

// s_waitcnt immediate that waits for vmcnt == n and ignores lgkm/exp (gfx9
// encoding: vmcnt[3:0] | vmcnt[5:4] << 14, expcnt[6:4], lgkmcnt[11:8])
constexpr int waitcnt_vmcnt(int n) {
  return (0xF << 8) | (0x7 << 4) | (n & 0xF) | (((n >> 4) & 0x3) << 14);
}

// K-split of an [M][K] weight whose kernel steps through K in slices of BK:
// fill the chip (>= 768 workgroups of 64 features) while every split keeps
// at least two steps. Launchers and the bindings (workspace size) both call
// this.
extern "C" int ks_skinny_nsplit(int M, int K, int BK);

// out[nm] bf16 = sum over nsplit of ws[nsplit][nm] bf16, accumulated in f32
// in split order
hipError_t ks_reduce_bf16_partials(short* out, const short* ws, long nm,
                                   int nsplit, hipStream_t stream);
