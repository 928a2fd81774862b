// Fused mixture-of-experts router: gate GEMM, top-k and the renormalised
// softmax weights in one launch (ops.moe_route).
//
//   logits[t][e] = sum_h x[t][h] * gate[e][h]      bf16 products, f32 sums
//   topi[t][0..k) = the k largest logits of row t, descending, ties to the
//                   LOWEST expert index (selection is on the logits, never on
//                   probabilities: two logits that differ may round to the same
//                   probability)
//   topw[t][j]    = exp(l_j - m) / sum_{selected} exp(l - m),  m = l_0
//
// which is softmax -> top-k -> renormalise with the full denominator cancelled.
// topi is int64 and topw f32, the tensors moe_align / the grouped GEMMs take.
//
// Work split: one workgroup per 16-token row tile (grid = ceil(T / 16), shapes
// only, so one capture serves any input). The x rows are the MFMA A operand,
// 16-expert column blocks of the gate the B operand, NB = E_pad / 16 blocks,
// 4 NB accumulator registers per wave. The waves split K: chunk c (32 wide,
// one v_mfma_f32_16x16x32_bf16 per block) belongs to wave c % NW, and a wave
// walks its chunks upwards. Both operands go straight from global memory to
// registers, 16 B per lane: x is read exactly once and the gate (<= 2 MB) lives
// in L2, so staging through LDS would add a write and a read per byte for no
// reuse. A wave loads D steps (one group) at a time, the next group as the
// MFMAs of the current one retire; D shrinks as NB grows so that everything
// stays in registers. A decode batch is a handful of workgroups and pure
// latency (one round trip per group), which is why there are 8 waves and,
// with the 16-expert gate, 8 steps per group: Mixtral's H = 4096 is two
// groups per wave.
//
// Clamping, not branching: rows past T load row T - 1, experts past E load
// gate row E - 1 and chunks past H / 32 load the last chunk; all are real
// addresses. Rows past T are never stored. Experts past E get the sentinel
// NEG before the top-k, so they can neither win a slot nor enter the sum
// (k <= E). A chunk past the end gets a zeroed A fragment, so it adds +0.
//
// Row invariance: MFMA rows do not mix, a wave adds its chunks in ascending
// order, and the epilogue adds the NW partial tiles from LDS in wave order
// 0..NW-1. Chunk ownership and NW depend on H and E alone, never on T or the
// grid, so a row's logits are the same bits wherever the row sits.
//
// Epilogue: the partial tiles are written to LDS in the MFMA C layout as they
// are (lane-contiguous, conflict free). In that layout the 16 experts of a
// block sit in the 16 lanes of a DPP row and a lane's four registers are four
// tokens; wave w < 4 takes register w of all four rows, i.e. tokens
// 4 * (lane >> 4) + w, and a lane holds the NB logits of experts
// 16 b + (lane & 15). Top-k is k rounds of (value, index) argmax: over the
// lane's own NB values, then four DPP steps across the row (quad xor 1, xor 2,
// half mirror, mirror) with "larger value, else lower index" as the order; the
// order is total, so all 16 lanes agree on the winner, and its owner masks it
// with NEG. Lane j keeps the j-th winner, then exp, a DPP row sum, one divide
// and one 8 B + one 4 B store per lane j < k.
//
// NEG is -FLT_MAX and not -inf: the tree builds with -ffast-math, which lets
// the compiler assume no infinities. exp is v_exp_f32 of (l - m) * log2(e):
// for a logit span of 23 the argument's rounding costs a relative 2^-19, the
// rest (exp, <= 8 terms, divide) a few ulp.
#include "common.h"
#include "mfma_layouts.h"

namespace {

constexpr int TILE_T = 16;      // tokens per workgroup
constexpr int CHUNK_K = 32;     // K of one MFMA: the kernel's K step
constexpr int MAX_EXPERTS = 256;
constexpr int MAX_TOPK = 8;
constexpr int EPI_WAVES = 4;    // one per C-layout register
constexpr float NEG = -3.4028234663852886e38f;

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

constexpr int DPP_QUAD_XOR1 = 0xB1;  // quad_perm:[1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;  // quad_perm:[2,3,0,1]
constexpr int DPP_ROW_HALF_MIRROR = 0x141;
constexpr int DPP_ROW_MIRROR = 0x140;

template <int CTRL>
__device__ __forceinline__ int dpp_mov(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, dpp_mov<CTRL>(__builtin_bit_cast(int, v)));
}

// (v, i) <- the better of it and the DPP partner's: larger value, else lower
// index. Partners exchange, so both end with the same pair.
template <int CTRL>
__device__ __forceinline__ void argmax_step(float& v, int& i) {
  const float ov = dpp_mov<CTRL>(v);
  const int oi = dpp_mov<CTRL>(i);
  const bool take = ov > v || (ov == v && oi < i);
  v = take ? ov : v;
  i = take ? oi : i;
}

// all-reduce over the 16 lanes of a DPP row; the four steps pair lanes like
// xor 1, 2, 4, 8 once the earlier steps have made quads / halves uniform
__device__ __forceinline__ void row_argmax(float& v, int& i) {
  argmax_step<DPP_QUAD_XOR1>(v, i);
  argmax_step<DPP_QUAD_XOR2>(v, i);
  argmax_step<DPP_ROW_HALF_MIRROR>(v, i);
  argmax_step<DPP_ROW_MIRROR>(v, i);
}

__device__ __forceinline__ float row_sum(float v) {
  v += dpp_mov<DPP_QUAD_XOR1>(v);
  v += dpp_mov<DPP_QUAD_XOR2>(v);
  v += dpp_mov<DPP_ROW_HALF_MIRROR>(v);
  v += dpp_mov<DPP_ROW_MIRROR>(v);
  return v;
}

// One K step of a wave: the A fragment of its 16 rows and NB B fragments.
template <int NB>
struct Frags {
  u32x4_t a;
  u32x4_t b[NB];
};

// NB   16-expert column blocks (E <= 16 NB)
// NW   waves per workgroup, all of which split K
// D    K steps per load group
template <int NB, int NW, int D>
__global__ __launch_bounds__(NW * WAVE_SIZE) void moe_route_kernel(
    long long* __restrict__ topi, float* __restrict__ topw,
    const short* __restrict__ x, const short* __restrict__ gate, int T, int H,
    int E, int top_k) {
  // partial logit tiles in C layout: [wave][reg][block][lane]
  __shared__ float part[NW * 4 * NB * WAVE_SIZE];

  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int rc = MFMA_RC_OF(lane);  // A row / B column, and the C column
  const int kgrp = lane >> 4;       // 8-element K group, and the C row group
  const long tile0 = (long)blockIdx.x * TILE_T;

  const int nchunks = H / CHUNK_K;
  const long row = min(tile0 + rc, (long)T - 1);
  const short* xp = x + row * H + kgrp * 8;
  const short* gp = gate + kgrp * 8;
  int goff[NB];  // E * H < 2^31 is checked on the host
#pragma unroll
  for (int b = 0; b < NB; ++b) goff[b] = min(b * 16 + rc, E - 1) * H;

  // step i of this wave is chunk wave + i * NW
  auto load = [&](int i, Frags<NB>& f) {
    const int k = min(wave + i * NW, nchunks - 1) * CHUNK_K;
    f.a = *(const u32x4_t*)(xp + k);
#pragma unroll
    for (int b = 0; b < NB; ++b) f.b[b] = *(const u32x4_t*)(gp + goff[b] + k);
  };

  f32x4_t acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int i, const Frags<NB>& f) {
    const bool valid = wave + i * NW < nchunks;  // wave-uniform
    const bf16x8_t a = __builtin_bit_cast(
        bf16x8_t, valid ? f.a : u32x4_t{0u, 0u, 0u, 0u});
#pragma unroll
    for (int b = 0; b < NB; ++b)
      acc[b] = mfma16x16x32(a, __builtin_bit_cast(bf16x8_t, f.b[b]), acc[b]);
  };

  // the trip count is that of wave 0, so every wave runs the same loop
  const int ngroups = cdiv(cdiv(nchunks, NW), D);
  Frags<NB> cur[D], nxt[D];
#pragma unroll
  for (int d = 0; d < D; ++d) load(d, cur[d]);
  for (int g = 0; g + 1 < ngroups; ++g) {
#pragma unroll
    for (int d = 0; d < D; ++d) load((g + 1) * D + d, nxt[d]);
#pragma unroll
    for (int d = 0; d < D; ++d) compute(g * D + d, cur[d]);
#pragma unroll
    for (int d = 0; d < D; ++d) cur[d] = nxt[d];
  }
#pragma unroll
  for (int d = 0; d < D; ++d) compute((ngroups - 1) * D + d, cur[d]);

#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      part[((wave * 4 + r) * NB + b) * WAVE_SIZE + lane] = acc[b][r];
  __syncthreads();
  if (wave >= EPI_WAVES) return;

  // this lane: token tile0 + 4 kgrp + wave, experts 16 b + rc
  float v[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    float s = part[(wave * NB + b) * WAVE_SIZE + lane];
#pragma unroll
    for (int w = 1; w < NW; ++w)
      s += part[((w * 4 + wave) * NB + b) * WAVE_SIZE + lane];
    v[b] = b * 16 + rc < E ? s : NEG;
  }

  float top = 0.f, my_v = 0.f;
  int my_i = 0;
  for (int j = 0; j < top_k; ++j) {
    float bv = v[0];
    int bi = rc;
#pragma unroll
    for (int b = 1; b < NB; ++b)
      if (v[b] > bv) bv = v[b], bi = b * 16 + rc;  // ascending index: ties stay
    row_argmax(bv, bi);
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (bi == b * 16 + rc) v[b] = NEG;
    if (j == 0) top = bv;
    if (j == rc) my_v = bv, my_i = bi;
  }
  const float p =
      rc < top_k
          ? __builtin_amdgcn_exp2f((my_v - top) * 1.4426950408889634f)
          : 0.f;
  const float w = p / row_sum(p);
  const long t = tile0 + kgrp * 4 + wave;
  if (t < T && rc < top_k) {
    topi[t * top_k + rc] = my_i;
    topw[t * top_k + rc] = w;
  }
}

template <int NB, int NW, int D>
void launch(void* topi, void* topw, const void* x, const void* gate, int T,
            int H, int E, int top_k, hipStream_t stream) {
  hipLaunchKernelGGL((moe_route_kernel<NB, NW, D>), dim3(cdiv(T, TILE_T)),
                     dim3(NW * WAVE_SIZE), 0, stream, (long long*)topi,
                     (float*)topw, (const short*)x, (const short*)gate, T, H, E,
                     top_k);
}

}  // namespace

// topi int64 [T][top_k], topw f32 [T][top_k] <- x bf16 [T][H], gate bf16
// [E][H]. Any T >= 1, 1 <= E <= 256, 1 <= top_k <= min(8, E), H % 32 == 0.
extern "C" hipError_t ks_moe_route(void* topi, void* topw, const void* x,
                                   const void* gate, int T, int H, int E,
                                   int top_k, hipStream_t stream) {
  if (T < 1 || E < 1 || E > MAX_EXPERTS || top_k < 1 || top_k > MAX_TOPK ||
      top_k > E || H <= 0 || H % CHUNK_K != 0 ||
      (long)E * H > 0x7fffffffL || T > 0x7fffffff - TILE_T)
    return hipErrorInvalidValue;
  // 16 B loads: rows are multiples of 64 B, so the bases decide
  if (((uintptr_t)x & 15) != 0 || ((uintptr_t)gate & 15) != 0 ||
      ((uintptr_t)topi & 7) != 0 || ((uintptr_t)topw & 3) != 0)
    return hipErrorInvalidValue;
  // LDS is NW * NB KB and the registers 2 D (NB + 1) + 5 NB quads, hence
  // fewer waves at 16 blocks and shallower groups as NB grows
  if (E <= 16) launch<1, 8, 8>(topi, topw, x, gate, T, H, E, top_k, stream);
  else if (E <= 32) launch<2, 8, 4>(topi, topw, x, gate, T, H, E, top_k, stream);
  else if (E <= 64) launch<4, 8, 2>(topi, topw, x, gate, T, H, E, top_k, stream);
  else if (E <= 128) launch<8, 8, 1>(topi, topw, x, gate, T, H, E, top_k, stream);
  else launch<16, 4, 1>(topi, topw, x, gate, T, H, E, top_k, stream);
  HIP_CHECK_KERNEL();
  return hipSuccess;
}
