// Batched multi-LoRA decode kernels (BGMV): every token row carries a
// device-side adapter slot, so one launch serves any adapter mix.
//
//   ks_lora_shrink:      tmp[t, 0:rr]  = sum_k x[t, k] * A[slot_t, 0:rr, k]
//   ks_lora_expand_add:  y[t, off + n] = bf16(float(y[t, off + n])
//                            + scale[slot_t] * sum_{r<rr} tmp[t, r] * B[slot_t, n, r])
//
// with rr = round_up(ranks[slot_t], 8). bf16 in, fp32 accumulate, fp32
// intermediate. The adapter matrices are tiny (rank 16 x K 4096 = 128 KiB)
// and L2-resident; at one row per adapter instance there is nothing for a
// matrix unit to reuse, so both kernels are vectorized FMA (16 B loads).
//
// Contract the engine and the tests rely on:
//  - The result of row t depends only on row t's inputs and its adapter's
//    weights: the work split and every summation order are functions of
//    (K, N, rr) alone. No atomics, no split across workgroups. A row gives
//    the same bits alone, in a mixed batch, eager or replayed from a graph.
//  - A row whose slot is < 0 or >= S is skipped: shrink writes nothing,
//    expand leaves y[t] untouched. Base-model rows and graph padding rows
//    carry -1, and a stale index can never become an out-of-range read.
//  - Only rows [0, rr) of A[slot] and columns [0, rr) of B[slot] are read.
//  - The launch functions neither allocate nor synchronize (capture-safe).
#include "common.h"

namespace {

constexpr int SHRINK_THREADS = 256;
constexpr int SHRINK_WAVES = SHRINK_THREADS / WAVE_SIZE;
constexpr int EXPAND_THREADS = 256;
constexpr int EXPAND_COLS = 4;  // y columns per thread (8 B accesses)

__device__ __forceinline__ int row_rank(const int* __restrict__ ranks,
                                        int slot, int R) {
  int r = ranks[slot];
  r = r < 0 ? 0 : r;
  int rr = (r + 7) & ~7;
  return rr > R ? R : rr;
}

// grid (R / 8, T), 256 threads. A workgroup owns 8 rank rows of one token
// row; its four waves stride over K in 2048-element steps (16 B per lane of
// x and of each A row), then reduce lanes by butterfly and waves through LDS
// in a fixed order.
__global__ void __launch_bounds__(SHRINK_THREADS)
lora_shrink_kernel(float* __restrict__ tmp,          // [T, R]
                   const short* __restrict__ x,      // [T, K], row stride
                   const short* __restrict__ a_stack,  // [S, R, K]
                   const int* __restrict__ slot_idx,   // [T]
                   const int* __restrict__ ranks,      // [S]
                   const int K, const int R, const int S,
                   const long x_stride) {
  __shared__ float s_part[SHRINK_WAVES][8];
  const int t = blockIdx.y;
  const int r0 = blockIdx.x * 8;
  const int slot = slot_idx[t];
  if (slot < 0 || slot >= S) return;  // uniform per workgroup
  if (r0 >= row_rank(ranks, slot, R)) return;

  const short* xrow = x + (size_t)t * x_stride;
  const short* arow = a_stack + ((size_t)slot * R + r0) * K;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;

  for (int k = threadIdx.x * 8; k < K; k += SHRINK_THREADS * 8) {
    const short8_t xv = *reinterpret_cast<const short8_t*>(xrow + k);
    float xf[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) xf[i] = bf16_bits_to_float(xv[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const short8_t av =
          *reinterpret_cast<const short8_t*>(arow + (size_t)j * K + k);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[j] += xf[i] * bf16_bits_to_float(av[i]);
    }
  }

  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = wave_reduce_sum(acc[j]);
    if (lane == 0) s_part[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    float v = s_part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < SHRINK_WAVES; ++w) v += s_part[w][threadIdx.x];
    tmp[(size_t)t * R + r0 + threadIdx.x] = v;
  }
}

// grid (ceil(N / 1024), T), 256 threads, four adjacent output columns per
// thread. tmp[t, 0:rr] is read as fp32 vectors at a wave-uniform address;
// each thread walks its four B rows 16 B at a time, r ascending.
__global__ void __launch_bounds__(EXPAND_THREADS)
lora_expand_add_kernel(short* __restrict__ y,            // [T, *], row stride
                       const float* __restrict__ tmp,    // [T, R]
                       const short* __restrict__ b_stack,  // [S, N, R]
                       const float* __restrict__ scale,    // [S]
                       const int* __restrict__ slot_idx,   // [T]
                       const int* __restrict__ ranks,      // [S]
                       const int N, const int R, const int S,
                       const long y_stride, const int off) {
  const int t = blockIdx.y;
  const int slot = slot_idx[t];
  if (slot < 0 || slot >= S) return;
  const int n0 = (blockIdx.x * EXPAND_THREADS + threadIdx.x) * EXPAND_COLS;
  if (n0 >= N) return;
  const int rr = row_rank(ranks, slot, R);
  const float sc = scale[slot];

  const float* trow = tmp + (size_t)t * R;
  const short* brow = b_stack + ((size_t)slot * N + n0) * R;
  float acc[EXPAND_COLS];
#pragma unroll
  for (int c = 0; c < EXPAND_COLS; ++c) acc[c] = 0.f;

  for (int r = 0; r < rr; r += 8) {
    const float4_t t0 = *reinterpret_cast<const float4_t*>(trow + r);
    const float4_t t1 = *reinterpret_cast<const float4_t*>(trow + r + 4);
#pragma unroll
    for (int c = 0; c < EXPAND_COLS; ++c) {
      const short8_t bv =
          *reinterpret_cast<const short8_t*>(brow + (size_t)c * R + r);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[c] += t0[i] * bf16_bits_to_float(bv[i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[c] += t1[i] * bf16_bits_to_float(bv[4 + i]);
      }
    }
  }

  short4_t* yp =
      reinterpret_cast<short4_t*>(y + (size_t)t * y_stride + off + n0);
  const short4_t yv = *yp;
  short4_t out;
#pragma unroll
  for (int c = 0; c < EXPAND_COLS; ++c)
    out[c] = float_to_bf16_bits(bf16_bits_to_float(yv[c]) + sc * acc[c]);
  *yp = out;
}

}  // namespace

extern "C" {

hipError_t ks_lora_shrink(void* tmp, const void* x, const void* a_stack,
                          const void* slot_idx, const void* ranks, int T,
                          int K, int R, int S, long x_stride,
                          hipStream_t stream) {
  if (K % 64 != 0 || R % 8 != 0 || K <= 0 || R <= 0 || S <= 0 ||
      x_stride % 8 != 0 || T > 65535)
    return hipErrorInvalidValue;
  if (T <= 0) return hipSuccess;
  hipLaunchKernelGGL(lora_shrink_kernel, dim3(R / 8, T), dim3(SHRINK_THREADS),
                     0, stream, (float*)tmp, (const short*)x,
                     (const short*)a_stack, (const int*)slot_idx,
                     (const int*)ranks, K, R, S, x_stride);
  HIP_CHECK_KERNEL();
  return hipSuccess;
}

hipError_t ks_lora_expand_add(void* y, const void* tmp, const void* b_stack,
                              const void* scale, const void* slot_idx,
                              const void* ranks, int T, int N, int R, int S,
                              long y_stride, int off, hipStream_t stream) {
  if (N % 64 != 0 || R % 8 != 0 || N <= 0 || R <= 0 || S <= 0 ||
      y_stride % 8 != 0 || off % 8 != 0 || off < 0 || T > 65535)
    return hipErrorInvalidValue;
  if (T <= 0) return hipSuccess;
  const int per_block = EXPAND_THREADS * EXPAND_COLS;
  hipLaunchKernelGGL(lora_expand_add_kernel,
                     dim3((N + per_block - 1) / per_block, T),
                     dim3(EXPAND_THREADS), 0, stream, (short*)y,
                     (const float*)tmp, (const short*)b_stack,
                     (const float*)scale, (const int*)slot_idx,
                     (const int*)ranks, N, R, S, y_stride, off);
  HIP_CHECK_KERNEL();
  return hipSuccess;
}
}
