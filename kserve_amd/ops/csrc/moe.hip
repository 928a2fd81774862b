// Routed mixture-of-experts MLP for decode-sized batches (bf16 in/out, f32
// accumulation): only the experts a batch routes to are read, the routing is
// taken from device tensors, and every grid depends on shapes alone, so one
// captured hipGraph serves any routing.
//
//   out[t] = bf16( sum_j topw[t][j] * down_e( bf16( silu(gate_e(x[t])) *
//                                                   up_e(x[t]) ) ) ),
//   e = topi[t][j] - expert_lo, pairs with e outside [0, E) dropped
//
// Four kernels, P = T * k pairs (pair id p = t * k + j):
//
//   1. align (one workgroup): LDS counting sort of the pairs by local expert.
//      offsets[E + 1] and sorted_pair[P]: pair ids grouped by expert, stable
//      in pair order. Ranks come from wave ballots and per-wave counters, so
//      no atomic decides an output position.
//   2. gate/up grouped GEMM + SiLU*mul: workgroup = (64 intermediate
//      features, expert, row chunk). Each wave streams 16 gate rows and the 16
//      matching up rows of w_gate_up[e], so the activation fuses in registers.
//      X rows are gathered through sorted_pair by the per-lane sources of
//      global_load_lds. Writes act[pos][I] bf16 at the row's SORTED position
//      (rounded once), so the down GEMM reads contiguous rows.
//   3. down grouped GEMM: workgroup = (64 hidden features, expert, row chunk,
//      K split). The epilogue multiplies by topw[pair] in f32 and writes
//      y[split][pair][H] f32 at the UNSORTED pair id.
//   4. combine: out[t] = bf16(sum_j sum_split y[split][t*k+j]) in that fixed
//      order. Dropped pairs are skipped by re-checking topi: their y rows are
//      never written and never read.
//
// Static grids and empty experts: the row-chunk dimension of the GEMM grids
// is ceil(T / chunk rows), the most rows one expert can hold (a token's k
// experts are distinct). A workgroup whose chunk starts at or past its
// expert's count exits before it touches a weight, so an unrouted expert
// costs a launch slot and no bytes. Inside a chunk, token tiles past the
// count skip their MFMAs wave-uniformly; ragged tiles clamp the row like
// skinny_gemm_kernel.
//
// Determinism and row independence: a row's dot products run over K in the
// same order whatever its position, tile or chunk (MFMA rows do not mix), the
// K split depends on I alone (ks_moe_nsplit), NT only changes how many rows
// share a workgroup, and the combine sums in fixed order. So the result is
// bit-identical from run to run, and permuting the input rows permutes the
// output rows bit for bit.
//
// W stream: straight to registers, as in wq_gemm.hip. With the token tile as
// the MFMA A operand and 16 features per wave as B, every W row is read by
// exactly one wave of one workgroup, so LDS would add a write and a read per
// W byte for no reuse; LDS is kept for the X tile, which all four waves
// share. The skinny_gemm.hip pattern (W through LDS) pays off when several
// waves consume the same W rows, which only happens here at T > 128 across
// row chunks, i.e. across workgroups, where LDS does not help either. A lane
// loads 2 x 16 B (16 consecutive K of its feature row) per step and stream,
// prefetched one step ahead of the MFMAs like the X tile; the gate/up kernel
// keeps 4 KB of W in flight per wave, the down kernel 2 KB and makes up for
// it with the K split's extra workgroups.
//
// K order, bf16: BK = 64. Lane (kgrp = lane >> 4) holds W elements k0 +
// kgrp*16 + [0, 16); MFMA kk in {0, 1} consumes elements kk*8..kk*8+7 of
// them, X chunk kc = kgrp*2 + kk. That is wq_gemm.hip's fp8 arrangement, so
// the X tile uses the same swizzle (derivation in wq_formats.h).
//
// Quantized experts (weight-only fp8 and MXFP4, kserve_amd/ops/quant.py):
// the GEMM kernel is a template over the weight format (MoeBf16, MoeFp8,
// MoeMxfp4 below). Both quantized formats run BK = 128 with KK = 4: a lane
// holds 32 consecutive K of its feature row, X chunk kc = kgrp*4 + kk, the
// 16-chunk X tile row takes Mxfp4::chunk_perm. The step is not the bf16 step
// with fewer bytes: fp8 keeps the bf16 kernel's 2 x 16 B per lane, stream and
// step (4 KB in flight per wave in gate/up) and covers twice the K with
// them; MXFP4 loads 16 B, exactly one MX block, plus that block's E8M0 scale
// byte, and applies the scale inside the convert. Converts are exact. The
// fp8 scale (one f32 per expert output row) multiplies the f32 accumulator
// in the epilogue: gate and up each by their own row's scale before
// SiLU*mul, down by scale * topw. At NT = 8 the double-buffered X tile is
// 64 KB, the static LDS limit.
//
// The rule above holds per format: k_per_split rounds up to the format's BK,
// so a row's summation order depends on the shapes and the format only.
#include "common.h"
#include "mfma_layouts.h"
#include "skinny_shared.h"
#include "wq_formats.h"

extern "C" int ks_moe_nsplit(int I);

namespace {

constexpr int FEAT_PER_WAVE = 16;
constexpr int NWAVES = 4;  // 64 features per workgroup

constexpr int MAX_TOKENS = 384;
constexpr int MAX_PAIRS = 768;
constexpr int MAX_TOPK = 8;
constexpr int MAX_EXPERTS = 256;  // local experts: 8 ballot bits, 1 thread each

// K split of the down GEMM: splits of at least 512 K (8 steps), at most 8 of
// them. A function of I alone, so a row's summation order is the same at
// every batch size.
constexpr int SPLIT_MIN_K = 512;
constexpr int MAX_SPLIT = 8;

// ---- weight formats of the grouped GEMMs ----
//
// BK, KK       K per step and MFMAs per step per token tile; a lane holds
//              BK/4 consecutive K of its feature row
// NLOAD        16 B register loads per lane, stream and step
// STEP_SCALE   one E8M0 scale byte per lane, stream and step (a VM
//              operation of its own), applied in the convert
// OUT_SCALE    one f32 scale per expert output row, applied in the epilogue
// row_bytes    bytes that k elements of a W row occupy
// chunk_perm   the format's part of the X tile swizzle (wq_formats.h)
// frag         the 8 bf16 of MFMA kk from a lane's registers of one step
struct MoeBf16 {
  static constexpr int BK = 64;
  static constexpr int KK = 2;
  static constexpr int NLOAD = 2;
  static constexpr bool STEP_SCALE = false;
  static constexpr bool OUT_SCALE = false;
  using scale_t = float;  // unused
  static __device__ __forceinline__ long row_bytes(long k) { return k * 2; }
  static __device__ __forceinline__ int chunk_perm(int kc) {
    return Fp8::chunk_perm(kc);
  }
  static __device__ __forceinline__ bf16x8_t frag(const u32x4_t (&w)[NLOAD],
                                                  int kk, float) {
    return __builtin_bit_cast(bf16x8_t, w[kk]);
  }
};

struct MoeFp8 {
  static constexpr int BK = 128;
  static constexpr int KK = 4;
  static constexpr int NLOAD = 2;
  static constexpr bool STEP_SCALE = false;
  static constexpr bool OUT_SCALE = true;
  using scale_t = float;
  static __device__ __forceinline__ long row_bytes(long k) { return k; }
  static __device__ __forceinline__ int chunk_perm(int kc) {
    return Mxfp4::chunk_perm(kc);
  }
  // 32 fp8 bytes in two loads: MFMA kk takes dwords 2*(kk&1), +1 of load kk/2
  static __device__ __forceinline__ bf16x8_t frag(const u32x4_t (&w)[NLOAD],
                                                  int kk, float) {
    return Fp8::cvt8(w[kk >> 1], kk & 1, 1.0f);
  }
};

struct MoeMxfp4 {
  static constexpr int BK = 128;
  static constexpr int KK = 4;
  static constexpr int NLOAD = 1;
  static constexpr bool STEP_SCALE = true;
  static constexpr bool OUT_SCALE = false;
  using scale_t = unsigned char;
  static __device__ __forceinline__ long row_bytes(long k) { return k / 2; }
  static __device__ __forceinline__ int chunk_perm(int kc) {
    return Mxfp4::chunk_perm(kc);
  }
  static __device__ __forceinline__ bf16x8_t frag(const u32x4_t (&w)[NLOAD],
                                                  int kk, float sc) {
    return Mxfp4::cvt8(w[0], kk, sc);
  }
};

// local expert of a routed id, or -1 (remote under EP, or not an expert)
__device__ __forceinline__ int local_expert(long long id, int expert_lo,
                                            int num_local) {
  const long long l = id - expert_lo;
  return (l >= 0 && l < num_local) ? (int)l : -1;
}

// ---- 1. align ----
//
// Wave w owns the pairs [w*per, (w+1)*per), in rounds of 64. In a round a
// lane's rank among the wave's earlier pairs of its expert is the wave's
// running count (LDS, private to the wave) plus the number of lower lanes in
// its match group; the highest lane of a group advances the count. After a
// scan over experts and waves the running counts become each wave's start
// inside its expert's segment.
__global__ __launch_bounds__(256) void moe_align_kernel(
    int* __restrict__ offsets,      // [E + 1]
    int* __restrict__ sorted_pair,  // [P]
    const long long* __restrict__ topi,  // [P]
    const int P, const int expert_lo, const int E) {
  __shared__ int wcnt[NWAVES][MAX_EXPERTS];
  __shared__ int total[MAX_EXPERTS];
  constexpr int ROUNDS = MAX_PAIRS / (NWAVES * 64);  // 3
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < NWAVES * MAX_EXPERTS; i += 256)
    (&wcnt[0][0])[i] = 0;
  __syncthreads();

  const int per = ((P + NWAVES * 64 - 1) / (NWAVES * 64)) * 64;
  int le[ROUNDS], rank[ROUNDS];
#pragma unroll
  for (int c = 0; c < ROUNDS; ++c) {
    const int p = wave * per + c * 64 + lane;
    int l = -1;
    if (c * 64 < per && p < P) l = local_expert(topi[p], expert_lo, E);
    unsigned long long m = __ballot(l >= 0);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (l >> b) & 1;
      const unsigned long long bb = __ballot(bit);
      m &= bit ? bb : ~bb;
    }
    le[c] = l;
    rank[c] = 0;
    if (l >= 0) {  // m = the lanes of this round with the same expert
      const int base = wcnt[wave][l];
      rank[c] = base + __popcll(m & ((1ull << lane) - 1ull));
      if ((m >> lane) == 1ull) wcnt[wave][l] = base + __popcll(m);
    }
    __syncthreads();
  }

  const int e = threadIdx.x;
  if (e < E) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) s += wcnt[w][e];
    total[e] = s;
  }
  __syncthreads();
  if (e < E) {
    int run = 0;
    for (int i = 0; i < e; ++i) run += total[i];
    offsets[e] = run;
    if (e == E - 1) offsets[E] = run + total[e];
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
      const int c = wcnt[w][e];
      wcnt[w][e] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < ROUNDS; ++c)
    if (le[c] >= 0)
      sorted_pair[wcnt[wave][le[c]] + rank[c]] = wave * per + c * 64 + lane;
}

// ---- 2, 3. grouped GEMMs ----
//
// NS W streams per wave: 2 (gate rows and up rows) or 1 (down rows).
// What one K-step of W occupies in a lane's registers; s is only written
// and read with STEP_SCALE.
template <class Fmt, int NS>
struct MoeRegs {
  u32x4_t w[NS][Fmt::NLOAD];
  unsigned int s[NS];
};

// grid: x = feature block of 64, y = local expert, z = chunk * nsplit + split
template <class Fmt, int NT, bool GATE_UP>
__global__ __launch_bounds__(256) void moe_gemm_kernel(
    short* __restrict__ act_out,  // GATE_UP: [P][N] bf16 by sorted position
    float* __restrict__ y_out,    // !GATE_UP: [nsplit][P][N] f32 by pair id
    const short* __restrict__ xin,  // GATE_UP: x [T][K]; else act [P][K]
    // GATE_UP: [E][2N] rows, else [E][N] rows, of row_bytes(K) each
    const unsigned char* __restrict__ w,
    // OUT_SCALE: f32 [E][2N] / [E][N]; STEP_SCALE: E8M0 [E][2N][K/32] /
    // [E][N][K/32]; bf16: unused
    const typename Fmt::scale_t* __restrict__ scale,
    const int* __restrict__ offsets, const int* __restrict__ sorted_pair,
    const float* __restrict__ topw,  // [P]
    const int N, const int K, const int P, const int top_k, const int nsplit,
    const int k_per_split) {
  constexpr int NS = GATE_UP ? 2 : 1;
  constexpr int BK = Fmt::BK;
  constexpr int ROW_CHUNKS = BK / 8;  // 16 B chunks in an X tile row
  using Regs = MoeRegs<Fmt, NS>;

  const int e = blockIdx.y;
  const int chunk = blockIdx.z / nsplit;
  const int split = blockIdx.z - chunk * nsplit;
  const int row_lo = offsets[e] + chunk * (NT * 16);
  // rows of this expert from this chunk on; the chunk holds min(rows, NT*16)
  const int rows = offsets[e + 1] - row_lo;
  if (rows <= 0) return;  // unrouted expert or unused chunk: no weight read

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int f_base = blockIdx.x * (NWAVES * FEAT_PER_WAVE);
  const int k_lo = split * k_per_split;
  const int k_hi = min(K, k_lo + k_per_split);

  // LDS: double-buffered X tile [NT*16][BK], swizzled; NINSTR wg-wide 1 KB
  // instructions, padded to NI per wave (NT = 1) into a dump slot.
  constexpr int NINSTR = NT * 16 * ROW_CHUNKS / 64;
  constexpr int NI = (NINSTR + NWAVES - 1) / NWAVES;
  constexpr bool PAD = NINSTR % NWAVES != 0;
  constexpr int TILE_SHORTS = NT * 16 * BK;
  __shared__ short tile[2][TILE_SHORTS];

  f32x4_t acc[NS][NT];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[s][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int m_local = lane & 15;
  const int kgrp = lane >> 4;
  // this lane's W streams: its feature row(s), NLOAD x 16 bytes per K-step
  // from K offset kgrp * BK/4, and with STEP_SCALE the scale byte of that
  // block (BK/4 = 32 = one MX block)
  const int frow = f_base + wave * FEAT_PER_WAVE + m_local;
  const unsigned char* wrow[NS];
  const unsigned char* srow[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const long row = ((long)e * NS + s) * N + frow;
    wrow[s] = w + row * Fmt::row_bytes(K) + Fmt::row_bytes(kgrp * (BK / 4));
    srow[s] = nullptr;
    if constexpr (Fmt::STEP_SCALE)
      srow[s] = scale + row * (K / 32) + kgrp;
  }

  // this lane's X sources, fixed over K: tile row -> sorted position ->
  // (GATE_UP) token of the pair there. Rows past the count clamp to the last.
  const short* xsrc[NI];
  short* xdst[NI];  // offset into tile[0]
#pragma unroll
  for (int ii = 0; ii < NI; ++ii) {
    const int i = wave + ii * NWAVES;
    const int g = i * 64 + lane;
    if (!PAD || i < NINSTR) {
      const int row = g / ROW_CHUNKS;
      const int kc_src = Fmt::chunk_perm((g & (ROW_CHUNKS - 1)) ^
                                    (row & (ROW_CHUNKS - 1)));
      const int pos = row_lo + min(row, rows - 1);
      const int src_row = GATE_UP ? sorted_pair[pos] / top_k : pos;
      xsrc[ii] = xin + (long)src_row * K + (kc_src << 3);
      xdst[ii] = &tile[0][i * 64 * 8];
    } else {  // padding instr keeps per-wave vmcnt uniform
      __shared__ short dump[512];
      xsrc[ii] = xin;
      xdst[ii] = dump;
    }
  }

  auto lds_row_idx = [](int row, int kc) {
    return (row * ROW_CHUNKS +
            (Fmt::chunk_perm(kc) ^ (row & (ROW_CHUNKS - 1)))) * 8;  // shorts
  };
  auto stage = [&](int buf, int k0) {
#pragma unroll
    for (int ii = 0; ii < NI; ++ii) {
      const int i = wave + ii * NWAVES;
      short* dst = xdst[ii];
      if (!PAD || i < NINSTR) dst += buf * TILE_SHORTS;
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const unsigned int*>(xsrc[ii] + k0),
          reinterpret_cast<unsigned int*>(dst), 16, 0, 0);
    }
  };
  auto load_w = [&](Regs& r, int k0) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const unsigned char* p = wrow[s] + Fmt::row_bytes(k0);
#pragma unroll
      for (int l = 0; l < Fmt::NLOAD; ++l)
        r.w[s][l] = *reinterpret_cast<const u32x4_t*>(p + l * 16);
      if constexpr (Fmt::STEP_SCALE) r.s[s] = srow[s][k0 / 32];
    }
  };

  // Per step a wave issues NW VM operations, in this order: per stream NLOAD
  // W register loads and, with STEP_SCALE, one scale byte load; then NI X
  // LDS loads. Waiting for NW outstanding means the whole previous step has
  // landed. A load added to the K loop is added here.
  constexpr int NW = NS * (Fmt::NLOAD + (Fmt::STEP_SCALE ? 1 : 0)) + NI;
  constexpr int WAIT_NEXT = waitcnt_vmcnt(NW);
  constexpr int WAIT_0 = waitcnt_vmcnt(0);

  auto compute = [&](const int buf, const Regs& use) {
    float sc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      sc[s] = 1.0f;
      if constexpr (Fmt::STEP_SCALE) sc[s] = e8m0_to_float(use.s[s]);
    }
#pragma unroll
    for (int kk = 0; kk < Fmt::KK; ++kk) {
      const int kc = kgrp * Fmt::KK + kk;
      bf16x8_t b[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) b[s] = Fmt::frag(use.w[s], kk, sc[s]);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (t * 16 < rows) {  // wave-uniform: tiles past the count do no work
          const bf16x8_t a = *reinterpret_cast<bf16x8_t*>(
              &tile[buf][lds_row_idx(t * 16 + m_local, kc)]);
#pragma unroll
          for (int s = 0; s < NS; ++s)
            acc[s][t] = mfma16x16x32(a, b[s], acc[s][t]);
        }
      }
    }
  };
  // a step with a successor (k0 + BK < k_hi): prefetch it, wait for step k0
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

  // straight-line body with the tail peeled, as in wq_gemm.hip
  Regs r_a{}, r_b{};
  int k0 = k_lo;
  if (k0 < k_hi) {
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

  // ---- epilogue: C row = tile row, col = feature ----
  // OUT_SCALE: each stream's accumulator takes its own row's scale in f32
  const int feat = f_base + wave * FEAT_PER_WAVE + MFMA_C_COL(lane);
  float osc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    osc[s] = 1.0f;
    if constexpr (Fmt::OUT_SCALE) osc[s] = scale[((long)e * NS + s) * N + feat];
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t * 16 >= rows) continue;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int r = t * 16 + MFMA_C_ROW(lane, reg);
      if (r < rows) {
        const int pos = row_lo + r;
        if constexpr (GATE_UP) {
          float g = acc[0][t][reg], u = acc[NS - 1][t][reg];
          if constexpr (Fmt::OUT_SCALE) {
            g *= osc[0];
            u *= osc[NS - 1];
          }
          const float a = g / (1.0f + __expf(-g)) * u;
          act_out[(long)pos * N + feat] = float_to_bf16_bits(a);
        } else {
          const int pair = sorted_pair[pos];
          float tw = topw[pair];
          if constexpr (Fmt::OUT_SCALE) tw *= osc[0];
          y_out[((long)split * P + pair) * N + feat] = acc[0][t][reg] * tw;
        }
      }
    }
  }
}

// ---- 4. combine: grid (T, ceil(H / 1024)), 4 features per thread ----
__global__ __launch_bounds__(256) void moe_combine_kernel(
    short* __restrict__ out,      // [T][H] bf16
    const float* __restrict__ y,  // [nsplit][P][H]
    const long long* __restrict__ topi, const int top_k, const int H,
    const int P, const int nsplit, const int expert_lo, const int E) {
  const int t = blockIdx.x;
  const int h = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (h >= H) return;
  float4_t s = float4_t{0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < top_k; ++j) {
    const int pair = t * top_k + j;
    if (local_expert(topi[pair], expert_lo, E) < 0) continue;
    for (int sp = 0; sp < nsplit; ++sp)
      s += *reinterpret_cast<const float4_t*>(
          y + ((long)sp * P + pair) * H + h);
  }
  short4_t o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = float_to_bf16_bits(s[i]);
  *reinterpret_cast<short4_t*>(out + (long)t * H + h) = o;
}

template <class Fmt, int NT>
void launch_gemms(short* act, float* y, const short* x,
                  const unsigned char* w_gate_up, const unsigned char* w_down,
                  const typename Fmt::scale_t* gate_up_scale,
                  const typename Fmt::scale_t* down_scale, const int* offsets,
                  const int* sorted_pair, const float* topw, int T, int top_k,
                  int H, int I, int E, int nsplit, int k_per_split,
                  hipStream_t stream) {
  const int P = T * top_k;
  const int nchunks = cdiv(T, NT * 16);
  hipLaunchKernelGGL((moe_gemm_kernel<Fmt, NT, true>),
                     dim3(I / 64, E, nchunks), dim3(256), 0, stream, act,
                     (float*)nullptr, x, w_gate_up, gate_up_scale, offsets,
                     sorted_pair, topw, I, H, P, top_k, 1, H);
  hipLaunchKernelGGL((moe_gemm_kernel<Fmt, NT, false>),
                     dim3(H / 64, E, nchunks * nsplit), dim3(256), 0, stream,
                     (short*)nullptr, y, act, w_down, down_scale, offsets,
                     sorted_pair, topw, H, I, P, top_k, nsplit, k_per_split);
}

// Workspaces (device): offsets int32 [E + 1], sorted_pair int32 [T*k], act
// bf16 [T*k][I], y f32 [ks_moe_nsplit(I)][T*k][H]. Nothing needs clearing.
template <class Fmt>
hipError_t moe_routed_mlp(void* out, const void* x, const void* topi,
                          const void* topw, const void* w_gate_up,
                          const void* w_down, const void* gate_up_scale,
                          const void* down_scale, void* offsets,
                          void* sorted_pair, void* act, void* y, int T,
                          int top_k, int H, int I, int E, int expert_lo,
                          hipStream_t stream) {
  constexpr int BK = Fmt::BK;
  // H and I are both a K and an N dimension: N needs % 64, K needs % BK
  static_assert(BK % (NWAVES * FEAT_PER_WAVE) == 0, "BK covers the N multiple");
  if (T < 1 || T > MAX_TOKENS || top_k < 1 || top_k > MAX_TOPK ||
      T * top_k > MAX_PAIRS || E < 1 || E > MAX_EXPERTS || H <= 0 ||
      H % BK != 0 || I <= 0 || I % BK != 0)
    return hipErrorInvalidValue;
  if ((Fmt::STEP_SCALE || Fmt::OUT_SCALE) &&
      (gate_up_scale == nullptr || down_scale == nullptr))
    return hipErrorInvalidValue;
  // 16-byte global_load_lds sources and W register loads; W rows are
  // multiples of 64 bytes in every format (K % BK == 0), so every row start
  // keeps the base alignment
  if (((uintptr_t)x & 15) != 0 || ((uintptr_t)act & 15) != 0 ||
      ((uintptr_t)w_gate_up & 15) != 0 || ((uintptr_t)w_down & 15) != 0 ||
      ((uintptr_t)y & 15) != 0 || ((uintptr_t)out & 7) != 0 ||
      (Fmt::OUT_SCALE && ((((uintptr_t)gate_up_scale) & 3) != 0 ||
                          (((uintptr_t)down_scale) & 3) != 0)))
    return hipErrorInvalidValue;
  const int P = T * top_k;
  const int nsplit = ks_moe_nsplit(I);
  const int k_per_split = ((I / nsplit + BK - 1) / BK) * BK;

  hipLaunchKernelGGL(moe_align_kernel, dim3(1), dim3(256), 0, stream,
                     (int*)offsets, (int*)sorted_pair, (const long long*)topi,
                     P, expert_lo, E);
#define CASE(nt)                                                           \
  launch_gemms<Fmt, nt>(                                                   \
      (short*)act, (float*)y, (const short*)x,                             \
      (const unsigned char*)w_gate_up, (const unsigned char*)w_down,       \
      (const typename Fmt::scale_t*)gate_up_scale,                         \
      (const typename Fmt::scale_t*)down_scale, (const int*)offsets,       \
      (const int*)sorted_pair, (const float*)topw, T, top_k, H, I, E,      \
      nsplit, k_per_split, stream)
  // rows per chunk = 16 * NT: the smallest tile count that holds T, up to 8
  if (T <= 16) CASE(1);
  else if (T <= 32) CASE(2);
  else if (T <= 64) CASE(4);
  else CASE(8);
#undef CASE
  hipLaunchKernelGGL(moe_combine_kernel, dim3(T, cdiv(H, 1024)), dim3(256), 0,
                     stream, (short*)out, (const float*)y,
                     (const long long*)topi, top_k, H, P, nsplit, expert_lo,
                     E);
  HIP_CHECK_KERNEL();
  return hipSuccess;
}

}  // namespace

extern "C" int ks_moe_nsplit(int I) {
  return max(1, min(MAX_SPLIT, I / SPLIT_MIN_K));
}

extern "C" hipError_t ks_moe_routed_mlp(
    void* out, const void* x, const void* topi, const void* topw,
    const void* w_gate_up, const void* w_down, void* offsets,
    void* sorted_pair, void* act, void* y, int T, int top_k, int H, int I,
    int E, int expert_lo, hipStream_t stream) {
  return moe_routed_mlp<MoeBf16>(out, x, topi, topw, w_gate_up, w_down,
                                 nullptr, nullptr, offsets, sorted_pair, act,
                                 y, T, top_k, H, I, E, expert_lo, stream);
}

// fp8 experts: codes [E][2I][H] / [E][H][I] e4m3, scales f32 [E][2I] / [E][H]
extern "C" hipError_t ks_moe_routed_mlp_w8(
    void* out, const void* x, const void* topi, const void* topw,
    const void* w_gate_up, const void* w_down, const void* gate_up_scale,
    const void* down_scale, void* offsets, void* sorted_pair, void* act,
    void* y, int T, int top_k, int H, int I, int E, int expert_lo,
    hipStream_t stream) {
  return moe_routed_mlp<MoeFp8>(out, x, topi, topw, w_gate_up, w_down,
                                gate_up_scale, down_scale, offsets,
                                sorted_pair, act, y, T, top_k, H, I, E,
                                expert_lo, stream);
}

// MXFP4 experts: codes [E][2I][H/2] / [E][H][I/2], E8M0 scales
// [E][2I][H/32] / [E][H][I/32]
extern "C" hipError_t ks_moe_routed_mlp_w4(
    void* out, const void* x, const void* topi, const void* topw,
    const void* w_gate_up, const void* w_down, const void* gate_up_scale,
    const void* down_scale, void* offsets, void* sorted_pair, void* act,
    void* y, int T, int top_k, int H, int I, int E, int expert_lo,
    hipStream_t stream) {
  return moe_routed_mlp<MoeMxfp4>(out, x, topi, topw, w_gate_up, w_down,
                                  gate_up_scale, down_scale, offsets,
                                  sorted_pair, act, y, T, top_k, H, I, E,
                                  expert_lo, stream);
}
