// Python bindings for the CDNA4 kernels (torch extension, ROCm-native:
// c10::hip stream APIs, no CUDA-compat shims).
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>

#include <hip/hip_runtime.h>

// launchers from the .hip translation units
extern "C" {
hipError_t ks_rms_norm(void*, const void*, const void*, float, int, int,
                       hipStream_t);
hipError_t ks_fused_add_rms_norm(void*, void*, const void*, float, int, int,
                                 hipStream_t);
hipError_t ks_silu_and_mul(void*, const void*, int, int, hipStream_t);
hipError_t ks_rotary_embedding(void*, void*, const void*, const void*, int,
                               int, int, int, long, long, hipStream_t);
hipError_t ks_reshape_and_cache(const void*, const void*, void*, void*,
                                const void*, int, int, int, int, long, long,
                                hipStream_t);
hipError_t ks_paged_attention_decode(void*, const void*, const void*,
                                     const void*, const void*, const void*,
                                     float, int, int, int, int, int, int,
                                     long, int, void*, void*, int,
                                     hipStream_t);
hipError_t ks_flash_prefill_varlen(void*, const void*, const void*,
                                   const void*, const void*, int, int, int,
                                   int, int, float, long, long, long, int,
                                   int, hipStream_t);
hipError_t ks_context_prefill_varlen(void*, const void*, const void*,
                                     const void*, const void*, const void*,
                                     const void*, int, int, int, int, int,
                                     int, float, long, int, int,
                                     hipStream_t);
hipError_t ks_paged_attention_decode_fp8(void*, const void*, const void*,
                                         const void*, const void*,
                                         const void*, float, int, int, int,
                                         int, int, int, long, int, void*,
                                         void*, int, hipStream_t);
hipError_t ks_reshape_and_cache_fp8(const void*, const void*, void*, void*,
                                    const void*, int, int, int, int, long,
                                    long, hipStream_t);
hipError_t ks_layer_norm(void*, const void*, const void*, const void*, float,
                         int, int, hipStream_t);
hipError_t ks_fused_add_layer_norm(void*, const void*, const void*,
                                   const void*, const void*, float, int, int,
                                   hipStream_t);
hipError_t ks_gelu(void*, const void*, long, hipStream_t);
hipError_t ks_greedy_sample(void*, const void*, int, int, hipStream_t);
hipError_t ks_gumbel_sample(void*, const void*, const void*, const void*,
                            const void*, int, int, hipStream_t);
hipError_t ks_topk_topp_sample(void*, const void*, const void*, const void*,
                               const void*, const void*, int, int,
                               hipStream_t);
hipError_t ks_topk_topp_minp_sample(void*, const void*, const void*,
                                    const void*, const void*, const void*,
                                    const void*, int, int, hipStream_t);
hipError_t ks_logit_process(void*, const void*, const void*, const void*,
                            const void*, const void*, const void*,
                            const void*, const void*, const void*, int, int,
                            int, int, hipStream_t);
hipError_t ks_token_count_add(void*, const void*, const void*, int, int, int,
                              hipStream_t);
hipError_t ks_mfma_probe(void*, const void*, const void*, hipStream_t);
hipError_t ks_skinny_gemm(void*, void*, const void*, const void*, int, int,
                          int, long, hipStream_t);
hipError_t ks_gemm8(void*, const void*, const void*, int, int, int, int,
                    hipStream_t);
int ks_skinny_nsplit(int, int, int);
hipError_t ks_skinny_gemm_w8(void*, void*, const void*, const void*,
                             const void*, int, int, int, long, hipStream_t);
hipError_t ks_skinny_gemm_w4(void*, void*, const void*, const void*,
                             const void*, int, int, int, long, hipStream_t);
hipError_t ks_dequant_mxfp4_rows(void*, const void*, const void*, long, int,
                                 hipStream_t);
hipError_t ks_dequant_fp8_rows(void*, const void*, const void*, long, int,
                               hipStream_t);
hipError_t ks_lora_shrink(void*, const void*, const void*, const void*,
                          const void*, int, int, int, int, long, hipStream_t);
hipError_t ks_lora_expand_add(void*, const void*, const void*, const void*,
                              const void*, const void*, int, int, int, int,
                              long, int, hipStream_t);
hipError_t ks_kv_gather_pages(void*, const void*, const void*, int, int, long,
                              int, int, int, int, hipStream_t);
hipError_t ks_kv_scatter_pages(const void*, const void*, const void*, int, int,
                               long, hipStream_t);
}

namespace {

hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

void check_hip(hipError_t err, const char* op) {
  TORCH_CHECK(err == hipSuccess, op, " failed: ", hipGetErrorString(err));
}

#define CHECK_BF16_CONTIG(t)                                       \
  TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bf16"); \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous");      \
  TORCH_CHECK((t).is_cuda(), #t " must be on GPU")

// [T, heads, D] where rows may be strided (qkv split views) but the
// (head, dim) block of each row is dense
#define CHECK_KV_CACHE(t)                                               \
  TORCH_CHECK((t).scalar_type() == at::kBFloat16 ||                       \
                  (t).scalar_type() == at::kFloat8_e4m3fn,                \
              #t " must be bf16 or fp8_e4m3");                            \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous");             \
  TORCH_CHECK((t).is_cuda(), #t " must be on GPU")

#define CHECK_BF16_ROWS(t)                                              \
  TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bf16");  \
  TORCH_CHECK((t).is_cuda(), #t " must be on GPU");                     \
  TORCH_CHECK((t).dim() == 3 && (t).stride(2) == 1 &&                   \
                  (t).stride(1) == (t).size(2),                         \
              #t " inner dims must be dense")

void rms_norm(at::Tensor& out, at::Tensor& input, at::Tensor& weight,
              double eps) {
  CHECK_BF16_CONTIG(out);
  CHECK_BF16_CONTIG(input);
  CHECK_BF16_CONTIG(weight);
  int hidden = input.size(-1);
  int rows = input.numel() / hidden;
  check_hip(ks_rms_norm(out.data_ptr(), input.data_ptr(), weight.data_ptr(),
                        (float)eps, rows, hidden, current_stream()),
            "rms_norm");
}

void fused_add_rms_norm(at::Tensor& x, at::Tensor& residual, at::Tensor& weight,
                        double eps) {
  CHECK_BF16_CONTIG(x);
  CHECK_BF16_CONTIG(residual);
  int hidden = x.size(-1);
  int rows = x.numel() / hidden;
  check_hip(
      ks_fused_add_rms_norm(x.data_ptr(), residual.data_ptr(),
                            weight.data_ptr(), (float)eps, rows, hidden,
                            current_stream()),
      "fused_add_rms_norm");
}

void silu_and_mul(at::Tensor& out, at::Tensor& input) {
  CHECK_BF16_CONTIG(out);
  CHECK_BF16_CONTIG(input);
  int d = out.size(-1);
  TORCH_CHECK(input.size(-1) == 2 * d, "input last dim must be 2*out");
  int rows = out.numel() / d;
  check_hip(ks_silu_and_mul(out.data_ptr(), input.data_ptr(), rows, d,
                            current_stream()),
            "silu_and_mul");
}

void rotary_embedding(at::Tensor& positions, at::Tensor& q, at::Tensor& k,
                      at::Tensor& cos_sin_cache) {
  CHECK_BF16_ROWS(q);
  CHECK_BF16_ROWS(k);
  TORCH_CHECK(positions.scalar_type() == at::kLong, "positions must be int64");
  TORCH_CHECK(cos_sin_cache.scalar_type() == at::kFloat,
              "cos_sin_cache must be fp32");
  int T = q.size(0);
  int Hq = q.size(1);
  int Hk = k.size(1);
  int D = q.size(2);
  check_hip(ks_rotary_embedding(q.data_ptr(), k.data_ptr(),
                                positions.data_ptr(), cos_sin_cache.data_ptr(),
                                T, Hq, Hk, D, (long)q.stride(0),
                                (long)k.stride(0), current_stream()),
            "rotary_embedding");
}

void reshape_and_cache(at::Tensor& k, at::Tensor& v, at::Tensor& k_cache,
                       at::Tensor& v_cache, at::Tensor& slot_mapping) {
  CHECK_BF16_ROWS(k);
  CHECK_BF16_ROWS(v);
  CHECK_KV_CACHE(k_cache);
  CHECK_KV_CACHE(v_cache);
  TORCH_CHECK(slot_mapping.scalar_type() == at::kInt, "slot_mapping int32");
  int T = k.size(0);
  int Hkv = k.size(1);
  int D = k.size(2);
  int block_size = k_cache.size(2);
  if (k_cache.scalar_type() == at::kFloat8_e4m3fn) {
    check_hip(ks_reshape_and_cache_fp8(k.data_ptr(), v.data_ptr(),
                                       k_cache.data_ptr(), v_cache.data_ptr(),
                                       slot_mapping.data_ptr(), T, Hkv, D,
                                       block_size, (long)k.stride(0),
                                       (long)v.stride(0), current_stream()),
              "reshape_and_cache_fp8");
    return;
  }
  check_hip(ks_reshape_and_cache(k.data_ptr(), v.data_ptr(),
                                 k_cache.data_ptr(), v_cache.data_ptr(),
                                 slot_mapping.data_ptr(), T, Hkv, D,
                                 block_size, (long)k.stride(0),
                                 (long)v.stride(0), current_stream()),
            "reshape_and_cache");
}

void paged_attention_decode(at::Tensor& out, at::Tensor& q,
                            at::Tensor& k_cache, at::Tensor& v_cache,
                            at::Tensor& block_tables, at::Tensor& context_lens,
                            double scale, int64_t window) {
  CHECK_BF16_CONTIG(out);
  CHECK_BF16_ROWS(q);
  CHECK_KV_CACHE(k_cache);
  CHECK_KV_CACHE(v_cache);
  TORCH_CHECK(block_tables.scalar_type() == at::kInt, "block_tables int32");
  TORCH_CHECK(context_lens.scalar_type() == at::kInt, "context_lens int32");
  // the kernels index both as dense arrays (row stride = size(1))
  TORCH_CHECK(block_tables.is_contiguous(), "block_tables must be contiguous");
  TORCH_CHECK(context_lens.is_contiguous(), "context_lens must be contiguous");
  const bool fp8 = k_cache.scalar_type() == at::kFloat8_e4m3fn;
  int S = q.size(0);
  int H = q.size(1);
  int D = q.size(2);
  int Hkv = k_cache.size(1);
  int block_size = k_cache.size(2);
  int max_blocks = block_tables.size(1);
  // split-context heuristic, measured A/B 2026-09-12 (gpurun_out/
  // attn_split_*.log): splitting HURTS at S>=256 (3.69->3.43 TB/s, the
  // fp32 partials + reduce outweigh extra waves) and for the group=8
  // HPW=2 shapes (2.05->1.81), but the 512-workgroup group<=4 regime
  // gains (S=64: 3.75->3.96 at 4 splits) and tiny batches need deep
  // splits (S=8: 0.71 unsplit vs 1.6-1.7 at 8-16). Rule: group<=4 AND
  // base<=512 -> clamp(2048/base, 2, 8); otherwise split only below
  // 512 workgroups (the round-1 rule).
  int n_splits = 1;
  long base_wgs = (long)S * Hkv;
  const int grp = H / Hkv;
  static const int split_override = [] {
    const char* e = getenv("KS_ATTN_SPLIT");
    return e ? atoi(e) : 0;  // 0 = heuristic
  }();
  if (split_override > 0) {
    n_splits = split_override;
  } else if (grp <= 4 && base_wgs <= 512) {
    n_splits = (int)(2048 / base_wgs);
    if (n_splits < 2) n_splits = 2;
    if (n_splits > 8) n_splits = 8;
  } else if (base_wgs < 512) {
    n_splits = (int)((512 + base_wgs - 1) / base_wgs);
    if (n_splits > 16) n_splits = 16;
  }
  if (n_splits > 1) {
    int max_split_blocks = (max_blocks + n_splits - 1) / n_splits;
    if (max_split_blocks < 1) n_splits = 1;
  }
  at::Tensor part_out, part_ml;
  void *po = nullptr, *pml = nullptr;
  if (n_splits > 1) {
    auto opts = at::TensorOptions().dtype(at::kFloat).device(q.device());
    part_out = at::empty({S, H, n_splits, D}, opts);
    part_ml = at::empty({S, H, n_splits, 2}, opts);
    po = part_out.data_ptr();
    pml = part_ml.data_ptr();
  }
  if (fp8) {
    TORCH_CHECK(H / Hkv <= 4 && D == 128,
                "fp8 KV decode supports D=128 and GQA group <= 4");
    check_hip(ks_paged_attention_decode_fp8(
                  out.data_ptr(), q.data_ptr(), k_cache.data_ptr(),
                  v_cache.data_ptr(), block_tables.data_ptr(),
                  context_lens.data_ptr(), (float)scale, S, H, Hkv, D,
                  max_blocks, block_size, (long)q.stride(0), n_splits, po,
                  pml, (int)window, current_stream()),
              "paged_attention_decode_fp8");
    return;
  }
  check_hip(ks_paged_attention_decode(
                out.data_ptr(), q.data_ptr(), k_cache.data_ptr(),
                v_cache.data_ptr(), block_tables.data_ptr(),
                context_lens.data_ptr(), (float)scale, S, H, Hkv, D,
                max_blocks, block_size, (long)q.stride(0), n_splits, po, pml,
                (int)window, current_stream()),
            "paged_attention_decode");
}

void flash_prefill_varlen(at::Tensor& out, at::Tensor& q, at::Tensor& k,
                          at::Tensor& v, at::Tensor& cu_seqlens,
                          int64_t max_seqlen, double scale,
                          bool causal = true, int64_t window = 0) {
  CHECK_BF16_CONTIG(out);
  CHECK_BF16_ROWS(q);
  CHECK_BF16_ROWS(k);
  CHECK_BF16_ROWS(v);
  TORCH_CHECK(cu_seqlens.scalar_type() == at::kInt, "cu_seqlens int32");
  int num_seqs = cu_seqlens.size(0) - 1;
  int Hq = q.size(1);
  int Hkv = k.size(1);
  int D = q.size(2);
  check_hip(ks_flash_prefill_varlen(out.data_ptr(), q.data_ptr(), k.data_ptr(),
                                    v.data_ptr(), cu_seqlens.data_ptr(),
                                    num_seqs, (int)max_seqlen, Hq, Hkv, D,
                                    (float)scale, (long)q.stride(0),
                                    (long)k.stride(0), (long)v.stride(0),
                                    causal ? 1 : 0, (int)window,
                                    current_stream()),
            "flash_prefill_varlen");
}

void context_prefill_varlen(at::Tensor& out, at::Tensor& q,
                            at::Tensor& k_cache, at::Tensor& v_cache,
                            at::Tensor& block_tables, at::Tensor& ctx_lens,
                            at::Tensor& cu_seqlens_q, int64_t max_q_len,
                            double scale, int64_t window) {
  CHECK_BF16_CONTIG(out);
  CHECK_BF16_ROWS(q);
  CHECK_KV_CACHE(k_cache);
  CHECK_KV_CACHE(v_cache);
  TORCH_CHECK(block_tables.scalar_type() == at::kInt, "block_tables int32");
  TORCH_CHECK(block_tables.is_contiguous(), "block_tables contiguous");
  TORCH_CHECK(ctx_lens.scalar_type() == at::kInt, "ctx_lens int32");
  TORCH_CHECK(cu_seqlens_q.scalar_type() == at::kInt, "cu_seqlens_q int32");
  TORCH_CHECK(k_cache.size(2) == 16, "block_size must be 16");
  int num_seqs = cu_seqlens_q.size(0) - 1;
  int Hq = q.size(1);
  int Hkv = k_cache.size(1);
  int D = q.size(2);
  int fp8 = k_cache.scalar_type() == at::kFloat8_e4m3fn ? 1 : 0;
  check_hip(ks_context_prefill_varlen(
                out.data_ptr(), q.data_ptr(), k_cache.data_ptr(),
                v_cache.data_ptr(), block_tables.data_ptr(),
                ctx_lens.data_ptr(), cu_seqlens_q.data_ptr(), num_seqs,
                (int)max_q_len, Hq, Hkv, D, (int)block_tables.size(1),
                (float)scale, (long)q.stride(0), fp8, (int)window,
                current_stream()),
            "context_prefill_varlen");
}

void layer_norm(at::Tensor& out, at::Tensor& input, at::Tensor& weight,
                at::Tensor& bias, double eps) {
  CHECK_BF16_CONTIG(out);
  CHECK_BF16_CONTIG(input);
  int hidden = input.size(-1);
  int rows = input.numel() / hidden;
  check_hip(ks_layer_norm(out.data_ptr(), input.data_ptr(), weight.data_ptr(),
                          bias.data_ptr(), (float)eps, rows, hidden,
                          current_stream()),
            "layer_norm");
}

void fused_add_layer_norm(at::Tensor& out, at::Tensor& input,
                          at::Tensor& residual, at::Tensor& weight,
                          at::Tensor& bias, double eps) {
  CHECK_BF16_CONTIG(out);
  CHECK_BF16_CONTIG(input);
  CHECK_BF16_CONTIG(residual);
  int hidden = input.size(-1);
  int rows = input.numel() / hidden;
  check_hip(ks_fused_add_layer_norm(out.data_ptr(), input.data_ptr(),
                                    residual.data_ptr(), weight.data_ptr(),
                                    bias.data_ptr(), (float)eps, rows, hidden,
                                    current_stream()),
            "fused_add_layer_norm");
}

void gelu(at::Tensor& out, at::Tensor& input) {
  CHECK_BF16_CONTIG(out);
  CHECK_BF16_CONTIG(input);
  check_hip(ks_gelu(out.data_ptr(), input.data_ptr(), input.numel(),
                    current_stream()),
            "gelu");
}

void greedy_sample(at::Tensor& out, at::Tensor& logits) {
  CHECK_BF16_CONTIG(logits);
  TORCH_CHECK(out.scalar_type() == at::kLong, "out int64");
  check_hip(ks_greedy_sample(out.data_ptr(), logits.data_ptr(),
                             logits.size(0), logits.size(1),
                             current_stream()),
            "greedy_sample");
}

void gumbel_sample(at::Tensor& out, at::Tensor& logits,
                   at::Tensor& temperatures, at::Tensor& top_k,
                   at::Tensor& seeds) {
  CHECK_BF16_CONTIG(logits);
  TORCH_CHECK(out.scalar_type() == at::kLong, "out int64");
  TORCH_CHECK(temperatures.scalar_type() == at::kFloat, "temps fp32");
  TORCH_CHECK(seeds.scalar_type() == at::kLong, "seeds int64");
  check_hip(ks_gumbel_sample(out.data_ptr(), logits.data_ptr(),
                             temperatures.data_ptr(), top_k.data_ptr(),
                             seeds.data_ptr(), logits.size(0), logits.size(1),
                             current_stream()),
            "gumbel_sample");
}

void topk_topp_sample(at::Tensor& out, at::Tensor& logits,
                      at::Tensor& temperatures, at::Tensor& top_p,
                      at::Tensor& top_k, at::Tensor& seeds) {
  CHECK_BF16_CONTIG(logits);
  TORCH_CHECK(out.scalar_type() == at::kLong, "out int64");
  TORCH_CHECK(temperatures.scalar_type() == at::kFloat, "temps fp32");
  TORCH_CHECK(top_p.scalar_type() == at::kFloat, "top_p fp32");
  TORCH_CHECK(top_k.scalar_type() == at::kInt, "top_k int32");
  TORCH_CHECK(seeds.scalar_type() == at::kLong, "seeds int64");
  check_hip(ks_topk_topp_sample(out.data_ptr(), logits.data_ptr(),
                                temperatures.data_ptr(), top_p.data_ptr(),
                                top_k.data_ptr(), seeds.data_ptr(),
                                logits.size(0), logits.size(1),
                                current_stream()),
            "topk_topp_sample");
}

// 1-D contiguous GPU tensor of `n` elements of dtype `ty`
#define CHECK_ROW_PARAM(t, ty, n)                                          \
  TORCH_CHECK((t).scalar_type() == (ty) && (t).is_cuda() &&                \
                  (t).dim() == 1 && (t).is_contiguous() &&                 \
                  (t).size(0) == (n),                                      \
              #t " must be a contiguous 1-D GPU tensor of " #ty " [" #n "]")

void topk_topp_minp_sample(at::Tensor& out, at::Tensor& logits,
                           at::Tensor& temperatures, at::Tensor& top_p,
                           at::Tensor& top_k, at::Tensor& min_p,
                           at::Tensor& seeds) {
  CHECK_BF16_CONTIG(logits);
  TORCH_CHECK(logits.dim() == 2, "logits must be [S, V]");
  const int64_t S = logits.size(0);
  CHECK_ROW_PARAM(out, at::kLong, S);
  CHECK_ROW_PARAM(temperatures, at::kFloat, S);
  CHECK_ROW_PARAM(top_p, at::kFloat, S);
  CHECK_ROW_PARAM(top_k, at::kInt, S);
  CHECK_ROW_PARAM(min_p, at::kFloat, S);
  CHECK_ROW_PARAM(seeds, at::kLong, S);
  check_hip(ks_topk_topp_minp_sample(
                out.data_ptr(), logits.data_ptr(), temperatures.data_ptr(),
                top_p.data_ptr(), top_k.data_ptr(), min_p.data_ptr(),
                seeds.data_ptr(), (int)S, (int)logits.size(1),
                current_stream()),
            "topk_topp_minp_sample");
}

// counts [slots, V] int32, contiguous, on the GPU
#define CHECK_TOKEN_COUNTS(t)                                              \
  TORCH_CHECK((t).scalar_type() == at::kInt && (t).is_cuda() &&            \
                  (t).dim() == 2 && (t).is_contiguous(),                   \
              #t " must be a contiguous int32 [slots, V] GPU tensor")

void logit_process(at::Tensor& out, at::Tensor& logits, at::Tensor& counts,
                   at::Tensor& row_slot, at::Tensor& presence,
                   at::Tensor& frequency, at::Tensor& repetition,
                   at::Tensor& bias_ids, at::Tensor& bias_vals,
                   at::Tensor& bias_len) {
  // out [S, V] bf16 <- bias then penalties on logits, per row from the slot
  // row_slot[s] of counts / bias_*; rows with a slot outside [0, slots) keep
  // their bits. out may be logits itself (in place).
  CHECK_BF16_CONTIG(logits);
  CHECK_BF16_CONTIG(out);
  TORCH_CHECK(logits.dim() == 2 && out.sizes() == logits.sizes(),
              "logits and out must both be [S, V]");
  const int64_t S = logits.size(0), V = logits.size(1);
  TORCH_CHECK(S <= 65535, "at most 65535 rows per call");
  const int64_t nbytes = S * V * 2;
  const char* lo = (const char*)logits.data_ptr();
  const char* oo = (const char*)out.data_ptr();
  TORCH_CHECK(oo == lo || oo + nbytes <= lo || lo + nbytes <= oo,
              "out must be logits itself or not overlap it");
  CHECK_TOKEN_COUNTS(counts);
  TORCH_CHECK(counts.size(1) == V, "counts must be [slots, V]");
  const int64_t slots = counts.size(0);
  CHECK_ROW_PARAM(row_slot, at::kInt, S);
  CHECK_ROW_PARAM(presence, at::kFloat, S);
  CHECK_ROW_PARAM(frequency, at::kFloat, S);
  CHECK_ROW_PARAM(repetition, at::kFloat, S);
  TORCH_CHECK(bias_ids.scalar_type() == at::kInt && bias_ids.is_cuda() &&
                  bias_ids.dim() == 2 && bias_ids.is_contiguous() &&
                  bias_ids.size(0) == slots,
              "bias_ids must be a contiguous int32 [slots, max_bias] GPU "
              "tensor");
  TORCH_CHECK(bias_vals.scalar_type() == at::kFloat && bias_vals.is_cuda() &&
                  bias_vals.is_contiguous() &&
                  bias_vals.sizes() == bias_ids.sizes(),
              "bias_vals must be a contiguous f32 [slots, max_bias] GPU "
              "tensor");
  CHECK_ROW_PARAM(bias_len, at::kInt, slots);
  check_hip(ks_logit_process(
                out.data_ptr(), logits.data_ptr(), counts.data_ptr(),
                row_slot.data_ptr(), presence.data_ptr(),
                frequency.data_ptr(), repetition.data_ptr(),
                bias_ids.data_ptr(), bias_vals.data_ptr(),
                bias_len.data_ptr(), (int)S, (int)V, (int)slots,
                (int)bias_ids.size(1), current_stream()),
            "logit_process");
}

void token_count_add(at::Tensor& counts, at::Tensor& slot,
                     at::Tensor& token) {
  // counts[slot[j], token[j]] += 1; out-of-range pairs skipped
  CHECK_TOKEN_COUNTS(counts);
  const int64_t n = slot.numel();
  CHECK_ROW_PARAM(slot, at::kInt, n);
  CHECK_ROW_PARAM(token, at::kLong, n);
  TORCH_CHECK(n < (int64_t)1 << 31 && counts.size(1) < (int64_t)1 << 31,
              "too many pairs or vocab entries");
  check_hip(ks_token_count_add(counts.data_ptr(), slot.data_ptr(),
                               token.data_ptr(), (int)n, (int)counts.size(0),
                               (int)counts.size(1), current_stream()),
            "token_count_add");
}

// bf16 partials for the kernel's K-split (each a full-precision-accumulated
// K/nsplit dot), sized by the policy the launchers use; undefined when the
// shape is not split. BK is the kernel's K step.
at::Tensor split_k_workspace(const at::Tensor& x, int N, int M, int K,
                             int BK) {
  const int nsplit = ks_skinny_nsplit(M, K, BK);
  if (nsplit <= 1) return at::Tensor();
  return at::empty({(long)nsplit * N * M},
                   at::TensorOptions().dtype(at::kBFloat16).device(x.device()));
}

void skinny_gemm(at::Tensor& out, at::Tensor& x, at::Tensor& w) {
  // out [N, M] bf16 = x [N, K] @ w [M, K]^T  (decode shapes, N <= 256)
  CHECK_BF16_CONTIG(out);
  CHECK_BF16_CONTIG(w);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.is_cuda() &&
                  x.stride(1) == 1,
              "x must be bf16 row-dense");
  int N = x.size(0);
  int K = x.size(1);
  int M = w.size(0);
  TORCH_CHECK(w.size(1) == K, "shape mismatch");
  at::Tensor ws = split_k_workspace(x, N, M, K, 64);
  check_hip(ks_skinny_gemm(out.data_ptr(), ws.defined() ? ws.data_ptr() : nullptr,
                           x.data_ptr(), w.data_ptr(), M, K, N,
                           (long)x.stride(0), current_stream()),
            "skinny_gemm");
}

#define CHECK_FP8_WEIGHT(q, scale)                                        \
  TORCH_CHECK((q).scalar_type() == at::kFloat8_e4m3fn && (q).is_cuda() && \
                  (q).dim() == 2 && (q).is_contiguous(),                  \
              #q " must be a contiguous 2-D fp8_e4m3fn GPU tensor");      \
  TORCH_CHECK((scale).scalar_type() == at::kFloat && (scale).is_cuda() && \
                  (scale).is_contiguous() &&                              \
                  (scale).numel() == (q).size(0),                         \
              #scale " must be f32 [out_features] on GPU")

// The weight-quantized decode GEMMs, after their own weight check: `gemm` is
// ks_skinny_gemm_w8 or _w4, wK the K that qweight holds, BK the kernel's K
// step, max_n its token limit.
void skinny_gemm_wq(const char* op, decltype(&ks_skinny_gemm_w8) gemm,
                    int64_t wK, int BK, int max_n, at::Tensor& out,
                    at::Tensor& x, at::Tensor& qweight, at::Tensor& scale) {
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.is_cuda() &&
                  x.dim() == 2 && x.stride(1) == 1,
              "x must be bf16 row-dense");
  int N = x.size(0);
  int K = x.size(1);
  int M = qweight.size(0);
  TORCH_CHECK(wK == K && out.dim() == 2 && out.size(0) == N &&
                  out.size(1) == M,
              "shape mismatch");
  TORCH_CHECK(N >= 1 && N <= max_n && M % 64 == 0 && K % BK == 0, op,
              " needs 1 <= N <= ", max_n, ", M % 64 == 0, K % ", BK, " == 0");
  at::Tensor ws = split_k_workspace(x, N, M, K, BK);
  check_hip(gemm(out.data_ptr(), ws.defined() ? ws.data_ptr() : nullptr,
                 x.data_ptr(), qweight.data_ptr(), scale.data_ptr(), M, K, N,
                 (long)x.stride(0), current_stream()),
            op);
}

void skinny_gemm_w8(at::Tensor& out, at::Tensor& x, at::Tensor& qweight,
                    at::Tensor& scale) {
  // out [N, M] bf16 = (x [N, K] bf16 @ qweight [M, K]^T e4m3) * scale [M]
  CHECK_BF16_CONTIG(out);
  CHECK_FP8_WEIGHT(qweight, scale);
  skinny_gemm_wq("skinny_gemm_w8", ks_skinny_gemm_w8, qweight.size(1), 64,
                 256, out, x, qweight, scale);
}

void dequant_fp8_rows(at::Tensor& out, at::Tensor& qweight,
                      at::Tensor& scale) {
  // out [M, K] bf16 = bf16(float(qweight [M, K] e4m3) * scale [M])
  CHECK_BF16_CONTIG(out);
  CHECK_FP8_WEIGHT(qweight, scale);
  TORCH_CHECK(out.numel() == qweight.numel(), "shape mismatch");
  check_hip(ks_dequant_fp8_rows(out.data_ptr(), qweight.data_ptr(),
                                scale.data_ptr(), (long)qweight.size(0),
                                (int)qweight.size(1), current_stream()),
            "dequant_fp8_rows");
}

// qweight uint8 [M, K/2] (two E2M1 codes per byte), scale uint8 [M, K/32]
// (E8M0), both contiguous; 16-byte aligned codes for the dwordx4 loads
#define CHECK_MXFP4_WEIGHT(q, scale)                                       \
  TORCH_CHECK((q).scalar_type() == at::kByte && (q).is_cuda() &&           \
                  (q).dim() == 2 && (q).is_contiguous() &&                 \
                  (q).size(1) % 16 == 0 &&                                 \
                  ((uintptr_t)(q).data_ptr() & 15) == 0,                   \
              #q " must be a contiguous, 16-byte aligned 2-D uint8 GPU "   \
                 "tensor [out, in/2] with in % 32 == 0");                  \
  TORCH_CHECK((scale).scalar_type() == at::kByte && (scale).is_cuda() &&   \
                  (scale).dim() == 2 && (scale).is_contiguous() &&         \
                  (scale).size(0) == (q).size(0) &&                        \
                  (scale).size(1) * 16 == (q).size(1),                     \
              #scale " must be uint8 [out, in/32] on GPU")

void skinny_gemm_w4(at::Tensor& out, at::Tensor& x, at::Tensor& qweight,
                    at::Tensor& scale) {
  // out [N, M] bf16 = x [N, K] bf16 @ dequant(qweight [M, K/2], scale)^T
  CHECK_BF16_CONTIG(out);
  CHECK_MXFP4_WEIGHT(qweight, scale);
  skinny_gemm_wq("skinny_gemm_w4", ks_skinny_gemm_w4, qweight.size(1) * 2,
                 128, 128, out, x, qweight, scale);
}

void dequant_mxfp4_rows(at::Tensor& out, at::Tensor& qweight,
                        at::Tensor& scale) {
  // out [M, K] bf16 = e2m1(qweight [M, K/2]) * 2^(scale [M, K/32] - 127)
  CHECK_BF16_CONTIG(out);
  CHECK_MXFP4_WEIGHT(qweight, scale);
  TORCH_CHECK(out.numel() == qweight.numel() * 2, "shape mismatch");
  TORCH_CHECK(((uintptr_t)out.data_ptr() & 15) == 0,
              "out must be 16-byte aligned");
  check_hip(ks_dequant_mxfp4_rows(out.data_ptr(), qweight.data_ptr(),
                                  scale.data_ptr(), (long)qweight.size(0),
                                  (int)qweight.size(1) * 2, current_stream()),
            "dequant_mxfp4_rows");
}

// [T, cols] bf16 rows of a possibly wider buffer: unit inner stride, every
// row start 16-byte aligned (the LoRA kernels use 16 B / 8 B vectors)
#define CHECK_LORA_ROWS(t)                                                 \
  TORCH_CHECK((t).scalar_type() == at::kBFloat16 && (t).is_cuda() &&       \
                  (t).dim() == 2,                                          \
              #t " must be a 2-D bf16 GPU tensor");                        \
  TORCH_CHECK((t).stride(1) == 1, #t " must have unit inner stride");      \
  TORCH_CHECK((t).size(0) <= 1 || (t).stride(0) % 8 == 0,                  \
              #t " row stride must be a multiple of 8 elements");          \
  TORCH_CHECK(reinterpret_cast<uintptr_t>((t).data_ptr()) % 16 == 0,       \
              #t " rows must be 16-byte aligned")

// stacks [S, rows, cols] bf16, per-slot scale/ranks, per-row slot index
void check_lora_meta(const at::Tensor& stack, const at::Tensor& ranks,
                     const at::Tensor& slot_idx, int64_t T) {
  TORCH_CHECK(stack.scalar_type() == at::kBFloat16 && stack.is_cuda() &&
                  stack.dim() == 3,
              "adapter stack must be a 3-D bf16 GPU tensor");
  TORCH_CHECK(stack.is_contiguous(), "adapter stack must be contiguous");
  TORCH_CHECK(ranks.scalar_type() == at::kInt && ranks.is_cuda() &&
                  ranks.is_contiguous() && ranks.dim() == 1 &&
                  ranks.size(0) == stack.size(0),
              "ranks must be a contiguous int32 [S] GPU tensor");
  TORCH_CHECK(slot_idx.scalar_type() == at::kInt && slot_idx.is_cuda() &&
                  slot_idx.dim() == 1 && slot_idx.size(0) == T,
              "slot_idx must be an int32 [T] GPU tensor");
  TORCH_CHECK(slot_idx.is_contiguous(), "slot_idx must be contiguous");
  TORCH_CHECK(T <= 65535, "at most 65535 rows per call");
}

void lora_shrink(at::Tensor& tmp, at::Tensor& x, at::Tensor& a_stack,
                 at::Tensor& ranks, at::Tensor& slot_idx) {
  // tmp [T, R] f32 <- x [T, K] bf16 . a_stack[slot_idx] [R, K]^T, rows with
  // a slot outside [0, S) skipped
  CHECK_LORA_ROWS(x);
  const int64_t T = x.size(0), K = x.size(1);
  check_lora_meta(a_stack, ranks, slot_idx, T);
  const int64_t S = a_stack.size(0), R = a_stack.size(1);
  TORCH_CHECK(a_stack.size(2) == K, "a_stack must be [S, R, K]");
  TORCH_CHECK(K > 0 && K % 64 == 0, "lora_shrink needs K % 64 == 0");
  TORCH_CHECK(R > 0 && R % 8 == 0, "lora_shrink needs R % 8 == 0");
  TORCH_CHECK(tmp.scalar_type() == at::kFloat && tmp.is_cuda() &&
                  tmp.is_contiguous() && tmp.dim() == 2 && tmp.size(0) == T &&
                  tmp.size(1) == R,
              "tmp must be a contiguous f32 [T, R] GPU tensor");
  check_hip(ks_lora_shrink(tmp.data_ptr(), x.data_ptr(), a_stack.data_ptr(),
                           slot_idx.data_ptr(), ranks.data_ptr(), (int)T,
                           (int)K, (int)R, (int)S,
                           T > 1 ? (long)x.stride(0) : 0L,
                           current_stream()),
            "lora_shrink");
}

void lora_expand_add(at::Tensor& y, at::Tensor& tmp, at::Tensor& b_stack,
                     at::Tensor& scale, at::Tensor& ranks,
                     at::Tensor& slot_idx, int64_t off) {
  // y[:, off:off+N] bf16 += scale[slot] * tmp [T, R] f32 . b_stack[slot]
  // [N, R]^T, in place, one rounding; rows with a slot outside [0, S) and
  // columns outside [off, off+N) untouched
  CHECK_LORA_ROWS(y);
  const int64_t T = y.size(0);
  check_lora_meta(b_stack, ranks, slot_idx, T);
  const int64_t S = b_stack.size(0), N = b_stack.size(1), R = b_stack.size(2);
  TORCH_CHECK(N > 0 && N % 64 == 0, "lora_expand_add needs N % 64 == 0");
  TORCH_CHECK(R > 0 && R % 8 == 0, "lora_expand_add needs R % 8 == 0");
  TORCH_CHECK(off >= 0 && off % 8 == 0,
              "out_offset must be a non-negative multiple of 8");
  TORCH_CHECK(off + N <= y.size(1), "out_offset + N exceeds the row of y");
  TORCH_CHECK(tmp.scalar_type() == at::kFloat && tmp.is_cuda() &&
                  tmp.is_contiguous() && tmp.dim() == 2 && tmp.size(0) == T &&
                  tmp.size(1) == R,
              "tmp must be a contiguous f32 [T, R] GPU tensor");
  TORCH_CHECK(scale.scalar_type() == at::kFloat && scale.is_cuda() &&
                  scale.is_contiguous() && scale.dim() == 1 &&
                  scale.size(0) == S,
              "scale must be a contiguous f32 [S] GPU tensor");
  check_hip(ks_lora_expand_add(y.data_ptr(), tmp.data_ptr(),
                               b_stack.data_ptr(), scale.data_ptr(),
                               slot_idx.data_ptr(), ranks.data_ptr(), (int)T,
                               (int)N, (int)R, (int)S,
                               T > 1 ? (long)y.stride(0) : 0L,
                               (int)off, current_stream()),
            "lora_expand_add");
}

// Shared checks of the KV export/import ops. `caches` is K0, V0, K1, V1, ...
// and `bases` the device table of their base pointers in the same order
// (built once by the caller); returns the bytes of one page of one tensor.
int64_t check_kv_transfer(const std::vector<at::Tensor>& caches,
                          at::Tensor& bases, at::Tensor& block_ids) {
  TORCH_CHECK(!caches.empty() && caches.size() % 2 == 0,
              "caches must list K and V of every layer");
  const at::Tensor& first = caches[0];
  TORCH_CHECK(first.dim() == 4, "cache must be [blocks, Hkv, block, D]");
  for (const at::Tensor& c : caches) {
    CHECK_KV_CACHE(c);
    TORCH_CHECK(c.scalar_type() == first.scalar_type() &&
                    c.sizes() == first.sizes() &&
                    c.device() == first.device(),
                "all layers must share one shape, dtype and device");
    TORCH_CHECK((uintptr_t)c.data_ptr() % 16 == 0,
                "caches must be 16-byte aligned");
  }
  TORCH_CHECK(bases.scalar_type() == at::kLong && bases.is_cuda() &&
                  bases.is_contiguous() && bases.dim() == 1 &&
                  bases.size(0) == (int64_t)caches.size(),
              "bases must be a contiguous int64 [2L] GPU tensor");
  TORCH_CHECK(block_ids.scalar_type() == at::kInt && block_ids.is_cuda() &&
                  block_ids.is_contiguous() && block_ids.dim() == 1,
              "block_ids must be a contiguous int32 [n] GPU tensor");
  const int64_t page_bytes = first.size(1) * first.size(2) * first.size(3) *
                             (int64_t)first.element_size();
  TORCH_CHECK(page_bytes % 16 == 0, "page bytes must be a multiple of 16");
  return page_bytes;
}

void kv_gather_pages(at::Tensor& out, std::vector<at::Tensor> caches,
                     at::Tensor& bases, at::Tensor& block_ids,
                     int64_t num_tokens) {
  // out [L, 2, n, Hkv, block, D] <- the listed pages of every cache; slots
  // at position >= num_tokens zeroed. out fp8 from bf16 pools converts.
  int64_t page_bytes = check_kv_transfer(caches, bases, block_ids);
  const at::Tensor& first = caches[0];
  CHECK_KV_CACHE(out);
  const bool convert = first.scalar_type() == at::kBFloat16 &&
                       out.scalar_type() == at::kFloat8_e4m3fn;
  TORCH_CHECK(convert || out.scalar_type() == first.scalar_type(),
              "payload dtype must equal the pool dtype, or be fp8_e4m3 for a "
              "bf16 pool (fp8 -> bf16 is refused)");
  TORCH_CHECK((uintptr_t)out.data_ptr() % 16 == 0,
              "out must be 16-byte aligned");
  if (convert) page_bytes /= 2;
  const int64_t row_bytes = first.size(3) * (int64_t)out.element_size();
  TORCH_CHECK(row_bytes % 16 == 0, "head_dim row must be a multiple of 16 B");
  const int64_t n = block_ids.size(0);
  const int64_t block_size = first.size(2);
  TORCH_CHECK(num_tokens >= 0 && num_tokens <= n * block_size,
              "num_tokens outside the listed pages");
  TORCH_CHECK(out.numel() == (int64_t)caches.size() * n * first.size(1) *
                                 block_size * first.size(3),
              "out must hold exactly [L, 2, n, Hkv, block, D] elements");
  check_hip(ks_kv_gather_pages(out.data_ptr(), bases.data_ptr(),
                               block_ids.data_ptr(), (int)caches.size(),
                               (int)n, (long)page_bytes, (int)row_bytes,
                               (int)block_size, (int)num_tokens,
                               convert ? 1 : 0, current_stream()),
            "kv_gather_pages");
}

void kv_scatter_pages(std::vector<at::Tensor> caches, at::Tensor& bases,
                      at::Tensor& block_ids, at::Tensor& src) {
  // the listed pages of every cache <- src [L, 2, n, Hkv, block, D]
  const int64_t page_bytes = check_kv_transfer(caches, bases, block_ids);
  const at::Tensor& first = caches[0];
  CHECK_KV_CACHE(src);
  TORCH_CHECK(src.scalar_type() == first.scalar_type(),
              "payload dtype must equal the pool dtype");
  TORCH_CHECK((uintptr_t)src.data_ptr() % 16 == 0,
              "src must be 16-byte aligned");
  const int64_t n = block_ids.size(0);
  TORCH_CHECK(src.numel() == (int64_t)caches.size() * n * first.size(1) *
                                 first.size(2) * first.size(3),
              "src must hold exactly [L, 2, n, Hkv, block, D] elements");
  check_hip(ks_kv_scatter_pages(src.data_ptr(), bases.data_ptr(),
                                block_ids.data_ptr(), (int)caches.size(),
                                (int)n, (long)page_bytes, current_stream()),
            "kv_scatter_pages");
}

void gemm8(at::Tensor& d, at::Tensor& a, at::Tensor& w, int64_t swizzle) {
  // EXPERIMENTAL (see gemm8.hip header): not used by ops.linear dispatch
  CHECK_BF16_CONTIG(d);
  CHECK_BF16_CONTIG(a);
  CHECK_BF16_CONTIG(w);
  int M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K && d.size(0) == M && d.size(1) == N,
              "shape mismatch");
  check_hip(ks_gemm8(d.data_ptr(), a.data_ptr(), w.data_ptr(), M, N, K,
                     (int)swizzle, current_stream()),
            "gemm8");
}

void mfma_probe(at::Tensor& c, at::Tensor& a, at::Tensor& b) {
  check_hip(ks_mfma_probe(c.data_ptr(), a.data_ptr(), b.data_ptr(),
                          current_stream()),
            "mfma_probe");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rms_norm", &rms_norm, "RMSNorm (bf16, CDNA4)");
  m.def("fused_add_rms_norm", &fused_add_rms_norm,
        "fused residual-add + RMSNorm, in-place");
  m.def("silu_and_mul", &silu_and_mul, "SwiGLU activation");
  m.def("rotary_embedding", &rotary_embedding, "neox RoPE in-place");
  m.def("reshape_and_cache", &reshape_and_cache, "KV page scatter");
  m.def("paged_attention_decode", &paged_attention_decode,
        "paged decode attention (GQA, split-context)");
  m.def("flash_prefill_varlen", &flash_prefill_varlen,
        "MFMA flash attention (varlen GQA, causal or bidirectional)",
        pybind11::arg("out"), pybind11::arg("q"), pybind11::arg("k"),
        pybind11::arg("v"), pybind11::arg("cu_seqlens"),
        pybind11::arg("max_seqlen"), pybind11::arg("scale"),
        pybind11::arg("causal") = true, pybind11::arg("window") = 0);
  m.def("context_prefill_varlen", &context_prefill_varlen,
        "MFMA prefill attention against the paged KV cache (chunked prefill)");
  m.def("layer_norm", &layer_norm, "LayerNorm (bf16)");
  m.def("fused_add_layer_norm", &fused_add_layer_norm,
        "residual-add + LayerNorm");
  m.def("gelu", &gelu, "erf GELU");
  m.def("greedy_sample", &greedy_sample, "argmax sampling");
  m.def("gumbel_sample", &gumbel_sample, "Gumbel-max temperature sampling");
  m.def("topk_topp_sample", &topk_topp_sample,
        "fused top-k/top-p + Gumbel-max sampler (radix-histogram select)");
  m.def("topk_topp_minp_sample", &topk_topp_minp_sample,
        "fused top-k/top-p/min-p + Gumbel-max sampler");
  m.def("logit_process", &logit_process,
        "logit_bias + presence/frequency/repetition penalties per row slot");
  m.def("token_count_add", &token_count_add,
        "counts[slot[j], token[j]] += 1 (atomic; out-of-range pairs skipped)");
  m.def("skinny_gemm", &skinny_gemm, "decode GEMM (N<=256, MFMA streaming)");
  m.def("skinny_gemm_w8", &skinny_gemm_w8,
        "decode GEMM, fp8 e4m3 weights x bf16 activations (N<=256)");
  m.def("dequant_fp8_rows", &dequant_fp8_rows,
        "fp8 e4m3 rows * per-row scale -> bf16");
  m.def("skinny_gemm_w4", &skinny_gemm_w4,
        "decode GEMM, MXFP4 weights x bf16 activations (N<=128)");
  m.def("dequant_mxfp4_rows", &dequant_mxfp4_rows,
        "MXFP4 rows (e2m1 codes, e8m0 block scales) -> bf16");
  m.def("lora_shrink", &lora_shrink,
        "batched multi-LoRA shrink: tmp = x . A[slot]^T per row (f32 out)");
  m.def("lora_expand_add", &lora_expand_add,
        "batched multi-LoRA expand: y += scale[slot] * tmp . B[slot]^T per row",
        pybind11::arg("y"), pybind11::arg("tmp"), pybind11::arg("b_stack"),
        pybind11::arg("scale"), pybind11::arg("ranks"),
        pybind11::arg("slot_idx"), pybind11::arg("out_offset") = 0);
  m.def("kv_gather_pages", &kv_gather_pages,
        "gather a request's KV pages of every layer into one buffer");
  m.def("kv_scatter_pages", &kv_scatter_pages,
        "scatter a gathered KV buffer into the listed pages of every layer");
  m.def("gemm8", &gemm8,
        "EXPERIMENTAL 8-phase 256x256 MFMA GEMM (round-2 candidate)");
  m.def("mfma_probe", &mfma_probe, "MFMA layout probe (tests)");
}
