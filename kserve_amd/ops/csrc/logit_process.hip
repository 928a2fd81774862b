// Logit processors for in-graph decode windows: logit_bias, then the
// presence / frequency / repetition penalties, applied per row from
// per-request device state (engine/logit_state.py), plus the token histogram
// update that follows sampling. Both are hipGraph-replayable: every input is
// device data, rows without processors carry slot -1 and are skipped.
//
// Per element, mirroring Sampler._apply_penalties (two bf16 roundings):
//   1. bias entry for the token:  x = bf16(float(x) + bias)
//   2. counts[slot, i] > 0:       v = float(x)
//                                 repetition != 1: v = v > 0 ? v / rep : v * rep
//                                 v = v - presence - frequency * count
//                                 x = bf16(v)
//   3. otherwise x keeps its bits.
#include "common.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_PER_THREAD = 8;
constexpr int LP_CHUNK = LP_THREADS * LP_PER_THREAD;  // vocab entries per block

typedef int int4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ short penalize(short bits, int count, float presence,
                                          float frequency, float repetition,
                                          bool use_rep) {
  if (count <= 0) return bits;
  float v = bf16_bits_to_float(bits);
  if (use_rep) v = v > 0.f ? v / repetition : v * repetition;
  v = v - presence - frequency * (float)count;
  return float_to_bf16_bits(v);
}

// grid (ceil(V / LP_CHUNK), S). The block's chunk of the row is staged in LDS
// so that the (few) bias entries that fall into it can be applied, by
// whichever thread reads them, before the element's owner penalizes it.
// VEC: V % 8 == 0 and all three base pointers 16-byte aligned, so every row
// start is too; the scalar variant takes any V and alignment.
template <bool VEC>
__global__ __launch_bounds__(LP_THREADS) void logit_process_kernel(
    short* out,           // [S, V] bf16; may be logits itself (no restrict)
    const short* logits,  // [S, V] bf16
    const int* __restrict__ counts,     // [slots, V]
    const int* __restrict__ row_slot,   // [S]
    const float* __restrict__ presence,    // [S]
    const float* __restrict__ frequency,   // [S]
    const float* __restrict__ repetition,  // [S]
    const int* __restrict__ bias_ids,      // [slots, max_bias]
    const float* __restrict__ bias_vals,   // [slots, max_bias]
    const int* __restrict__ bias_len,      // [slots]
    const int V, const int slots, const int max_bias) {
  const int s = blockIdx.y;
  const int c0 = blockIdx.x * LP_CHUNK;
  const int tid = threadIdx.x;
  const int slot = row_slot[s];
  const short* in_row = logits + (long)s * V;
  short* out_row = out + (long)s * V;
  const int n_here = min(LP_CHUNK, V - c0);

  if (slot < 0 || slot >= slots) {
    // no processors: in place nothing happens, out of place the row is copied
    if (out != logits) {
      if constexpr (VEC) {
        const int i = c0 + tid * LP_PER_THREAD;
        if (i < V)
          *reinterpret_cast<short8_t*>(out_row + i) =
              *reinterpret_cast<const short8_t*>(in_row + i);
      } else {
        for (int j = tid; j < n_here; j += LP_THREADS)
          out_row[c0 + j] = in_row[c0 + j];
      }
    }
    return;
  }

  __shared__ short tile[LP_CHUNK];
  if constexpr (VEC) {
    const int j = tid * LP_PER_THREAD;
    if (j < n_here)
      *reinterpret_cast<short8_t*>(tile + j) =
          *reinterpret_cast<const short8_t*>(in_row + c0 + j);
  } else {
    for (int j = tid; j < n_here; j += LP_THREADS) tile[j] = in_row[c0 + j];
  }
  __syncthreads();

  // bias first (ids are unique within a slot, so no two threads meet)
  int nb = bias_len[slot];
  nb = nb < 0 ? 0 : (nb > max_bias ? max_bias : nb);
  const int* ids = bias_ids + (long)slot * max_bias;
  const float* vals = bias_vals + (long)slot * max_bias;
  for (int b = tid; b < nb; b += LP_THREADS) {
    const int j = ids[b] - c0;
    if (j >= 0 && j < n_here)
      tile[j] = float_to_bf16_bits(bf16_bits_to_float(tile[j]) + vals[b]);
  }
  __syncthreads();

  const float p = presence[s];
  const float f = frequency[s];
  const float r = repetition[s];
  const bool use_rep = r != 1.0f;
  const int* cnt_row = counts + (long)slot * V + c0;
  if constexpr (VEC) {
    const int j = tid * LP_PER_THREAD;
    if (j < n_here) {
      short8_t x = *reinterpret_cast<const short8_t*>(tile + j);
      const int4_t ca = *reinterpret_cast<const int4_t*>(cnt_row + j);
      const int4_t cb = *reinterpret_cast<const int4_t*>(cnt_row + j + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        x[e] = penalize(x[e], ca[e], p, f, r, use_rep);
        x[e + 4] = penalize(x[e + 4], cb[e], p, f, r, use_rep);
      }
      *reinterpret_cast<short8_t*>(out_row + c0 + j) = x;
    }
  } else {
    for (int j = tid; j < n_here; j += LP_THREADS)
      out_row[c0 + j] = penalize(tile[j], cnt_row[j], p, f, r, use_rep);
  }
}

// counts[slot[j], token[j]] += 1; pairs with a slot outside [0, slots) or a
// token outside [0, V) are skipped. Duplicate pairs all count (atomic add).
__global__ __launch_bounds__(256) void token_count_add_kernel(
    int* __restrict__ counts,         // [slots, V]
    const int* __restrict__ slot,     // [n]
    const long* __restrict__ token,   // [n]
    const int n, const int slots, const int V) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int sl = slot[j];
  const long t = token[j];
  if (sl < 0 || sl >= slots || t < 0 || t >= (long)V) return;
  atomicAdd(counts + (long)sl * V + t, 1);
}

}  // namespace

extern "C" {

hipError_t ks_logit_process(void* out, const void* logits, const void* counts,
                            const void* row_slot, const void* presence,
                            const void* frequency, const void* repetition,
                            const void* bias_ids, const void* bias_vals,
                            const void* bias_len, int num_seqs, int vocab,
                            int slots, int max_bias, hipStream_t stream) {
  if (num_seqs == 0 || vocab == 0) return hipSuccess;
  const dim3 grid((vocab + LP_CHUNK - 1) / LP_CHUNK, num_seqs);
  const bool vec = (vocab % 8 == 0) && ((uintptr_t)out % 16 == 0) &&
                   ((uintptr_t)logits % 16 == 0) &&
                   ((uintptr_t)counts % 16 == 0);
  if (vec) {
    hipLaunchKernelGGL((logit_process_kernel<true>), grid, dim3(LP_THREADS), 0,
                       stream, (short*)out, (const short*)logits,
                       (const int*)counts, (const int*)row_slot,
                       (const float*)presence, (const float*)frequency,
                       (const float*)repetition, (const int*)bias_ids,
                       (const float*)bias_vals, (const int*)bias_len, vocab,
                       slots, max_bias);
  } else {
    hipLaunchKernelGGL((logit_process_kernel<false>), grid, dim3(LP_THREADS),
                       0, stream, (short*)out, (const short*)logits,
                       (const int*)counts, (const int*)row_slot,
                       (const float*)presence, (const float*)frequency,
                       (const float*)repetition, (const int*)bias_ids,
                       (const float*)bias_vals, (const int*)bias_len, vocab,
                       slots, max_bias);
  }
  HIP_CHECK_KERNEL();
  return hipSuccess;
}

hipError_t ks_token_count_add(void* counts, const void* slot,
                              const void* token, int n, int slots, int vocab,
                              hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(token_count_add_kernel, dim3((n + 255) / 256), dim3(256),
                     0, stream, (int*)counts, (const int*)slot,
                     (const long*)token, n, slots, vocab);
  HIP_CHECK_KERNEL();
  return hipSuccess;
}
}
