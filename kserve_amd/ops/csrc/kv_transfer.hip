// KV page export / import for prefill-decode disaggregation.
//
// A request's pages are scattered over the paged cache, once per layer and
// once each for K and V. Gather copies them, for every layer and both
// tensors in ONE launch, into a contiguous buffer
//   [L, 2, n, Hkv, block_size, D]
// and scatter writes such a buffer back into the listed pages of another
// pool. Cache layout is the one of kv_cache.hip: [num_blocks, Hkv,
// block_size, D] per tensor, one page (Hkv*block_size*D items) contiguous.
//
// Work is flat over 16-byte vectors of the contiguous side: vector i belongs
// to item i / page_vecs (item = tensor*n + j, tensor = 2*layer + is_v, which
// is also the order of the base-pointer table) and sits at i % page_vecs
// inside the page. The grid is capped and strides over the remainder.
//
// The kernels do not bounds-check block ids; the Python wrapper validates
// them on the host before anything is launched.
#include "common.h"

namespace {

typedef unsigned int uint4_t __attribute__((ext_vector_type(4)));

constexpr int KV_THREADS = 256;
constexpr int KV_MAX_GRID = 2048;

// Token slot of a page-relative row: the page is [Hkv, block_size, row] and
// rows are whole multiples of a vector, so a vector lies in one slot.
__device__ __forceinline__ int slot_of(unsigned int vec, unsigned int row_vecs,
                                       unsigned int block_size) {
  return (int)((vec / row_vecs) % block_size);
}

// Same-dtype gather. Slots at logical position >= num_tokens are written as
// zero bytes: the tail of a request's last page may still hold an earlier
// request's K/V, which must not leave the process.
__global__ __launch_bounds__(KV_THREADS) void kv_gather_pages_kernel(
    uint4_t* __restrict__ out,            // [2L, n, page_vecs]
    const long long* __restrict__ bases,  // [2L] K0, V0, K1, V1, ...
    const int* __restrict__ block_ids,    // [n]
    const unsigned int n, const unsigned int page_vecs,
    const unsigned int row_vecs, const unsigned int block_size,
    const int num_tokens, const unsigned int total_vecs) {
  const unsigned int stride = gridDim.x * KV_THREADS;
  for (unsigned int i = blockIdx.x * KV_THREADS + threadIdx.x; i < total_vecs;
       i += stride) {
    const unsigned int item = i / page_vecs;
    const unsigned int vec = i - item * page_vecs;
    const unsigned int tensor = item / n;
    const unsigned int j = item - tensor * n;
    uint4_t val = {0u, 0u, 0u, 0u};
    const int pos = (int)(j * block_size) + slot_of(vec, row_vecs, block_size);
    if (pos < num_tokens) {
      const uint4_t* src = reinterpret_cast<const uint4_t*>(bases[tensor]);
      val = src[(long)block_ids[j] * page_vecs + vec];
    }
    out[i] = val;
  }
}

// bf16 pool -> fp8 E4M3 payload. One 16-byte output vector holds 16 values,
// read as two short8 loads. Conversion, scale (1.0) and pairing are those of
// reshape_and_cache_fp8_kernel (kv_cache.hip), so every byte equals what an
// fp8 pool would have stored for the same bf16 value.
__global__ __launch_bounds__(KV_THREADS) void kv_gather_pages_fp8_kernel(
    uint4_t* __restrict__ out,            // [2L, n, page_vecs] (fp8 bytes)
    const long long* __restrict__ bases,  // bf16 pools
    const int* __restrict__ block_ids, const unsigned int n,
    const unsigned int page_vecs,  // per OUTPUT page
    const unsigned int row_vecs, const unsigned int block_size,
    const int num_tokens, const unsigned int total_vecs) {
  const unsigned int stride = gridDim.x * KV_THREADS;
  for (unsigned int i = blockIdx.x * KV_THREADS + threadIdx.x; i < total_vecs;
       i += stride) {
    const unsigned int item = i / page_vecs;
    const unsigned int vec = i - item * page_vecs;
    const unsigned int tensor = item / n;
    const unsigned int j = item - tensor * n;
    uint4_t val = {0u, 0u, 0u, 0u};
    const int pos = (int)(j * block_size) + slot_of(vec, row_vecs, block_size);
    if (pos < num_tokens) {
      const short8_t* src = reinterpret_cast<const short8_t*>(bases[tensor]);
      const long at = ((long)block_ids[j] * page_vecs + vec) * 2;
      const short8_t lo = src[at];
      const short8_t hi = src[at + 1];
      // the builtin's word-select must be a literal; unroll by hand
#define CVT2(dst_, a, b, w)                \
  dst_ = __builtin_amdgcn_cvt_pk_fp8_f32(  \
      bf16_bits_to_float(a), bf16_bits_to_float(b), dst_, w)
      unsigned int p0 = 0, p1 = 0, p2 = 0, p3 = 0;
      CVT2(p0, lo[0], lo[1], false);
      CVT2(p0, lo[2], lo[3], true);
      CVT2(p1, lo[4], lo[5], false);
      CVT2(p1, lo[6], lo[7], true);
      CVT2(p2, hi[0], hi[1], false);
      CVT2(p2, hi[2], hi[3], true);
      CVT2(p3, hi[4], hi[5], false);
      CVT2(p3, hi[6], hi[7], true);
#undef CVT2
      val = uint4_t{p0, p1, p2, p3};
    }
    out[i] = val;
  }
}

// Inverse of the same-dtype gather: whole pages, zero tail included, into
// exactly the listed pages of the destination pool.
__global__ __launch_bounds__(KV_THREADS) void kv_scatter_pages_kernel(
    const uint4_t* __restrict__ src,      // [2L, n, page_vecs]
    const long long* __restrict__ bases,  // [2L] destination pools
    const int* __restrict__ block_ids, const unsigned int n,
    const unsigned int page_vecs, const unsigned int total_vecs) {
  const unsigned int stride = gridDim.x * KV_THREADS;
  for (unsigned int i = blockIdx.x * KV_THREADS + threadIdx.x; i < total_vecs;
       i += stride) {
    const unsigned int item = i / page_vecs;
    const unsigned int vec = i - item * page_vecs;
    const unsigned int tensor = item / n;
    const unsigned int j = item - tensor * n;
    uint4_t* dst = reinterpret_cast<uint4_t*>(bases[tensor]);
    dst[(long)block_ids[j] * page_vecs + vec] = src[i];
  }
}

// total 16-byte vectors of the contiguous buffer, or 0 if the shape is not
// one the kernels index with 32 bits
unsigned int total_vecs_of(int num_tensors, int n, long page_bytes) {
  if (num_tensors <= 0 || n <= 0 || page_bytes <= 0 || page_bytes % 16 != 0)
    return 0;
  const long long total = (long long)num_tensors * n * (page_bytes / 16);
  if (total >= (1LL << 31) || page_bytes / 16 >= (1LL << 31)) return 0;
  return (unsigned int)total;
}

int grid_for(unsigned int total_vecs) {
  const unsigned int blocks = (total_vecs + KV_THREADS - 1) / KV_THREADS;
  return (int)(blocks < (unsigned int)KV_MAX_GRID ? blocks : KV_MAX_GRID);
}

}  // namespace

// out_page_bytes / row_bytes describe the OUTPUT (payload) side; with
// convert_fp8 the pools hold bf16 and the payload one byte per value.
extern "C" hipError_t ks_kv_gather_pages(void* out, const void* bases,
                                         const void* block_ids,
                                         int num_tensors, int n,
                                         long out_page_bytes, int row_bytes,
                                         int block_size, int num_tokens,
                                         int convert_fp8,
                                         hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const unsigned int total = total_vecs_of(num_tensors, n, out_page_bytes);
  if (total == 0 || row_bytes <= 0 || row_bytes % 16 != 0 || block_size <= 0 ||
      out_page_bytes % ((long)row_bytes * block_size) != 0)
    return hipErrorInvalidValue;
  const unsigned int page_vecs = (unsigned int)(out_page_bytes / 16);
  const unsigned int row_vecs = (unsigned int)(row_bytes / 16);
  if (convert_fp8) {
    hipLaunchKernelGGL(kv_gather_pages_fp8_kernel, dim3(grid_for(total)),
                       dim3(KV_THREADS), 0, stream, (uint4_t*)out,
                       (const long long*)bases, (const int*)block_ids,
                       (unsigned int)n, page_vecs, row_vecs,
                       (unsigned int)block_size, num_tokens, total);
  } else {
    hipLaunchKernelGGL(kv_gather_pages_kernel, dim3(grid_for(total)),
                       dim3(KV_THREADS), 0, stream, (uint4_t*)out,
                       (const long long*)bases, (const int*)block_ids,
                       (unsigned int)n, page_vecs, row_vecs,
                       (unsigned int)block_size, num_tokens, total);
  }
  HIP_CHECK_KERNEL();
  return hipSuccess;
}

extern "C" hipError_t ks_kv_scatter_pages(const void* src, const void* bases,
                                          const void* block_ids,
                                          int num_tensors, int n,
                                          long page_bytes,
                                          hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const unsigned int total = total_vecs_of(num_tensors, n, page_bytes);
  if (total == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kv_scatter_pages_kernel, dim3(grid_for(total)),
                     dim3(KV_THREADS), 0, stream, (const uint4_t*)src,
                     (const long long*)bases, (const int*)block_ids,
                     (unsigned int)n, (unsigned int)(page_bytes / 16), total);
  HIP_CHECK_KERNEL();
  return hipSuccess;
}
