// PyTorch bindings for the gfx950 kernels.  The kernels themselves are plain HIP compiled by
// hipcc (no torch headers); this translation unit validates tensors, picks the current HIP
// stream (so every op is hipGraph-capturable) and calls the C launchers.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <cmath>

#include "gemm_dec_forms.h"
#include "gemm_skinny_plan.h"
#include "gemm_tile_forms.h"
#include "paged_decode_forms.h"

extern "C" {
int k8sllm_rmsnorm(void* out, const void* x, void* residual, const void* w, long rows, int d, float eps,
                   long x_stride, long out_stride, hipStream_t s);
int k8sllm_layernorm(void* out, const void* x, const void* w, const void* b, long rows, int d, float eps,
                     hipStream_t s);
int k8sllm_silu_mul(void* out, const void* x, long rows, int F, int pairing, hipStream_t s);
int k8sllm_gelu_tanh(void* out, const void* x, long n, hipStream_t s);
int k8sllm_embedding(void* out, const int* ids, const void* weight, long T, int d, int vocab_start, int rows,
                     hipStream_t s);
int k8sllm_resolve_ids(int* out, const int* ids, const int* src, const int* prev, int n, hipStream_t s);
int k8sllm_rope_cache(void* qkv, long qkv_stride, const int* positions, const float* cos_sin, void* k_cache,
                      void* v_cache, const int* slot_mapping, long T, int Hq, int Hkv, int D, int block_size,
                      int apply_rope, const float* partial, int S, float* kv_scale, const void* q_norm_w,
                      const void* k_norm_w, float eps, int norm_bf16, hipStream_t s);
int k8sllm_paged_decode(void* out, long out_stride, float* part_out, float* part_ml, const void* q, long q_stride,
                        void* k_cache, void* v_cache, const int* block_tables, int bt_stride, const int* seq_lens,
                        int B, int Hq, int Hkv, int D, int S, float scale, float* kv_scale, const float* slabs,
                        int nslabs, const int* positions, const float* cos_sin, const int* slot_mapping,
                        int* merge_ctr, hipStream_t s);
int k8sllm_paged_decode_forms(int* out, int cap);
void k8sllm_decode_tw_force(int tw);
int k8sllm_flash_prefill(void* out, long out_stride, const void* qkv, long qkv_stride, const int* cu_seqlens,
                         const int* qb_seq, const int* qb_start, int n_qblocks, int Hq, int Hkv, int D, float scale,
                         const int* ctx_start, const void* k_cache, const void* v_cache, const int* block_tables,
                         int bt_stride, const float* kv_scale, hipStream_t s);
int k8sllm_sample(int* out, const void* logits, int is_fp32, long B, long stride, int V, const float* temps,
                  const int* top_k, const float* top_p, const int64_t* rng, float* pv, int* pi, int advance, hipStream_t s);
int k8sllm_sample_pen(int* out, const void* logits, int is_fp32, long B, long stride, int V, const float* temps,
                      const int* top_k, const float* top_p, const int64_t* rng, float* pv, int* pi, int advance,
                      const int* pslot, void* table, long tstride, const float* pparams, int nslots, hipStream_t s);
int k8sllm_sample_guided(int* out, const void* logits, int is_fp32, long B, long stride, int V, const float* temps,
                         const int* top_k, const float* top_p, const int64_t* rng, float* pv, int* pi, int advance,
                         const int* pslot, void* table, long tstride, const float* pparams, int nslots,
                         const int* gslot, int* gstate, int gnslots, const void* gmask, int gW, const int* gtrans,
                         int grows, const int* tok_off, const void* blob, const int* eos_ids, int n_eos, hipStream_t s);
int k8sllm_guide_mask_build(void* mask, int W, const int* trans, const void* accept, int* popc, const int* rows, int n,
                            int nrows, const int* tok_off, const void* blob, int V, const int* eos_ids, int n_eos,
                            hipStream_t s);
int k8sllm_penalty_reset(void* table, long tstride, int V, int nslots, int slot, const int* ids, int n_prompt,
                         int n_out, float* pparams, float rep, float inv_rep, float presence, float frequency,
                         hipStream_t s);
int k8sllm_sample_parts(long B, int V);
long k8sllm_token_logprobs_ws(long B, int V);
int k8sllm_token_logprobs(int* out, const void* logits, int is_fp32, long B, long stride, int V, const int* tok,
                          const int* want, void* ws, hipStream_t s);
int k8sllm_pool_l2(float* out, const void* x, int is_fp32, const int* dim, long rows, int d, long x_stride,
                   hipStream_t s);
int k8sllm_moe_route(const void* logits, long T, int E, int K, int renorm, int* topk_ids, float* topk_w,
                     hipStream_t s);
int k8sllm_moe_router(const void* x, const void* wr, long T, int d, int E, int K, int renorm, int* ids, float* w,
                      float* wd, hipStream_t s);
int k8sllm_moe_align(const int* topk_ids, long n, int E, int* expert_offsets, int* sorted_idx, int* inv_idx,
                     hipStream_t s);
int k8sllm_moe_combine(void* out, const void* expert_out, const int* inv_idx, const float* topk_w, long T, int K,
                       int d, hipStream_t s);
int k8sllm_gather_rows(void* out, const void* x, const int* idx, long n, int d, int div, hipStream_t s);
int k8sllm_gemm_tile(const void* X, const void* W, void* Y, int M, int N, int K, const int* offsets, int E, long w_es,
                     int epi, int algo, const int* rope_pos, const float* rope_cs, int rope_heads,
                     const float* rs_part, int rs_np, float rs_eps, void* resid, void* hw, const void* norm_w,
                     float* ss_out, int wpk, const void* wscale, int wfmt, int persist, int cus, hipStream_t s);
int k8sllm_gemm_tile_forms(int* out, int cap);
int k8sllm_gemm_tile_persist_forms(int* out, int cap);
int k8sllm_moe_grouped_gemm(const void* X, const void* W, void* Y, const int* offsets, int E, long rows, int N, int K,
                            long w_es, int epi, hipStream_t s);
int k8sllm_gemm_skinny(const void* A, long lda, const void* Wp, float* partial, void* Y, long ldy, int M, int N, int K,
                       int S, int epi, int nt_tiles, int a_packed, const float* rn_ss, int rn_nc, int rn_d,
                       float rn_eps, int waves, int experts, long w_es, long a_es, long y_es,
                       const float* row_w, int row_w_ld, int w_rm, hipStream_t s);
int k8sllm_gemm_dec(const void* A, const void* W, const void* wscale, int wf, float* partial, void* Y, long ldy, int M,
                    int N, int K, int splits, int epi, int ntw, int waves, int depth, int f4_depth, const float* rn_ss,
                    int rn_nc, int rn_d, float rn_eps, int experts, long a_es, long w_eb, long s_eb, long y_es,
                    const float* rw, int rw_ld, int sw_rows, int sw_wt, int sw_xcd, const float* delta, const int* dslot,
                    int nslots, hipStream_t s);
int k8sllm_gemm_dec_forms(int* out, int cap);
int k8sllm_gemm_dec_f8_forms(int* out, int cap);
int k8sllm_gemm_dec_f4_forms(int* out, int cap);
int k8sllm_gemm_dec_rc(const void* A, const void* Wp, void* resid, const void* nw, void* xw, float* ss, int M, int N,
                       int K, hipStream_t s);
int k8sllm_add_norm_partial(void* out, long out_stride, void* residual, const float* partial, int S, int M,
                            const void* w, int d, float* ss_part, hipStream_t s);
int k8sllm_embed_norm_partial(void* out, long out_stride, void* residual, const int* ids, const int* src,
                              const int* prev, const void* emb, int vocab, const void* w, int M, int d,
                              float* ss_part, hipStream_t s);
int k8sllm_reduce_slabs(void* out, const float* partial, int S, long n, hipStream_t s);
int k8sllm_lora_shrink_plan(int K);
int k8sllm_lora_shrink(const void* x, int packed, long xstride, const void* A, const int* slot, const float* ss_part,
                       int ss_cols, float eps, float* t_part, long M, int R, int K, int nslots, hipStream_t s);
int k8sllm_lora_expand(const float* t_part, int S, const void* B, const float* scaling, const int* slot, float* slab,
                       void* y, long ystride, long M, int N, int R, int nslots, hipStream_t s);
int k8sllm_reduce_add_rmsnorm(void* out, void* residual, const float* partial, int S, int M, const void* w, int d,
                              float eps, long out_stride, void* out2, hipStream_t s);
void* k8sllm_car_create(int rank, int world, long max_elems, void* handles, int* err);
int k8sllm_car_handle_size();
int k8sllm_car_open(void* state, const void* all_handles);
int k8sllm_car_all_reduce(void* state, const void* in, void* out, long n, long spin_limit, int algo, hipStream_t s);
int k8sllm_car_fused_tail(void* state, const float* slabs, int ns, long slab_stride, void* residual, const void* w,
                          void* out, long ldo, int M, int d, float eps, int packed, long spin_limit, int algo,
                          hipStream_t s);
int k8sllm_car_error(void* state);
int k8sllm_car_all_gather(void* state, const void* in, void* out, long n, long spin_limit, hipStream_t s);
int k8sllm_car_all_to_all(void* state, const void* in, void* out, long n, long spin_limit, hipStream_t s);
int k8sllm_car_error_async(void* state, void* host_dst, hipStream_t s);
void k8sllm_car_destroy(void* state);
}

namespace {

hipStream_t cur() { return c10::hip::getCurrentHIPStream().stream(); }

void check(int rc, const char* what) { TORCH_CHECK(rc == 0, "k8sllm kernel launch failed: ", what, " rc=", rc); }

void dev_bf16(const torch::Tensor& t, const char* n) {
  TORCH_CHECK(t.is_cuda(), n, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, n, " must be bfloat16");
}

void dev_i32(const torch::Tensor& t, const char* n) {
  TORCH_CHECK(t.is_cuda(), n, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kInt32, n, " must be int32");
  TORCH_CHECK(t.is_contiguous(), n, " must be contiguous");
}

void rms_norm(torch::Tensor out, torch::Tensor x, torch::Tensor w, double eps) {
  dev_bf16(out, "out"); dev_bf16(x, "x"); dev_bf16(w, "w");
  const int d = (int)x.size(-1);
  TORCH_CHECK(x.stride(-1) == 1 && out.stride(-1) == 1 && w.is_contiguous(), "rms_norm: inner dim must be contiguous");
  const long rows = x.numel() / d;
  const long xs = x.dim() > 1 ? x.stride(-2) : d, os = out.dim() > 1 ? out.stride(-2) : d;
  check(k8sllm_rmsnorm(out.data_ptr(), x.data_ptr(), nullptr, w.data_ptr(), rows, d, (float)eps, xs, os, cur()),
        "rms_norm");
}

void fused_add_rms_norm(torch::Tensor out, torch::Tensor x, torch::Tensor residual, torch::Tensor w, double eps) {
  dev_bf16(out, "out"); dev_bf16(x, "x"); dev_bf16(residual, "residual"); dev_bf16(w, "w");
  TORCH_CHECK(residual.is_contiguous() && w.is_contiguous() && x.stride(-1) == 1, "fused_add_rms_norm layout");
  const int d = (int)x.size(-1);
  const long rows = x.numel() / d;
  TORCH_CHECK(residual.numel() == rows * d, "residual shape");
  const long xs = x.dim() > 1 ? x.stride(-2) : d, os = out.dim() > 1 ? out.stride(-2) : d;
  check(k8sllm_rmsnorm(out.data_ptr(), x.data_ptr(), residual.data_ptr(), w.data_ptr(), rows, d, (float)eps, xs, os,
                       cur()),
        "fused_add_rms_norm");
}

// The paged KV cache of one layer: bf16 (no scales), or e4m3 codes in the same index order with
// kv_scale [NB, Hkv, 2, 16] fp32 (ops.kv_cache_alloc; head_dim 128, 16-token blocks).  Returns the
// scales pointer (nullptr for bf16).
float* kv_cache_pair(const torch::Tensor& k_cache, const torch::Tensor& v_cache,
                     const c10::optional<torch::Tensor>& kv_scale, int64_t Hkv, int64_t D) {
  if (k_cache.scalar_type() != torch::kFloat8_e4m3fn) {
    dev_bf16(k_cache, "k_cache"); dev_bf16(v_cache, "v_cache");
    TORCH_CHECK(!kv_scale.has_value(), "kv_scale goes with an e4m3 cache");
    return nullptr;
  }
  TORCH_CHECK(k_cache.is_cuda() && v_cache.is_cuda() && v_cache.scalar_type() == torch::kFloat8_e4m3fn,
              "fp8 KV cache: k_cache and v_cache must both be e4m3 GPU tensors");
  TORCH_CHECK(D == 128, "fp8 KV cache: head_dim 128 only");
  TORCH_CHECK(kv_scale.has_value(), "fp8 KV cache needs kv_scale");
  TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous() && k_cache.dim() == 5 && v_cache.dim() == 4 &&
                  k_cache.size(1) == Hkv && k_cache.size(2) == D / 8 && k_cache.size(3) == 16 && k_cache.size(4) == 8 &&
                  v_cache.size(0) == k_cache.size(0) && v_cache.size(1) == Hkv && v_cache.size(2) == D &&
                  v_cache.size(3) == 16,
              "fp8 KV cache: caches [NB, Hkv, D/8, 16, 8] / [NB, Hkv, D, 16]");
  TORCH_CHECK(kv_scale->is_cuda() && kv_scale->scalar_type() == torch::kFloat32 && kv_scale->is_contiguous() &&
                  kv_scale->dim() == 4 && kv_scale->size(0) == k_cache.size(0) && kv_scale->size(1) == Hkv &&
                  kv_scale->size(2) == 2 && kv_scale->size(3) == 16,
              "fp8 KV cache: kv_scale [NB, Hkv, 2, 16] fp32");
  return kv_scale->data_ptr<float>();
}

void layer_norm(torch::Tensor out, torch::Tensor x, torch::Tensor w, torch::Tensor b, double eps) {
  dev_bf16(out, "out"); dev_bf16(x, "x"); dev_bf16(w, "w"); dev_bf16(b, "b");
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous(), "layer_norm: contiguous");
  const int d = (int)x.size(-1);
  check(k8sllm_layernorm(out.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), x.numel() / d, d, (float)eps, cur()),
        "layer_norm");
}

// interleaved: x columns are [64 gate | 64 up] per 128 (ops.interleave_gate_up) instead of [F | F]
// pairing of gate and up inside x [.., 2F]: 0 [F gate | F up], 1 [64 gate | 64 up] per 128 columns,
// 8 [8 gate | 8 up] per 16 (the row order of a PACKED w13, ops.interleave_gate_up8)
void silu_mul_pairing(torch::Tensor out, torch::Tensor x, int64_t pairing) {
  dev_bf16(out, "out"); dev_bf16(x, "x");
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous(), "silu_mul: contiguous");
  const int F = (int)out.size(-1);
  TORCH_CHECK(x.size(-1) == 2 * F, "silu_mul: x last dim must be 2*F");
  TORCH_CHECK(pairing == 0 || pairing == 1 || pairing == 8, "silu_mul: pairing 0, 1 (per 128 columns) or 8 (per 16)");
  TORCH_CHECK(pairing != 1 || F % 64 == 0, "silu_mul: interleaved gate/up needs F % 64 == 0");
  check(k8sllm_silu_mul(out.data_ptr(), x.data_ptr(), out.numel() / F, F, (int)pairing, cur()), "silu_mul");
}

void silu_mul(torch::Tensor out, torch::Tensor x, bool interleaved) { silu_mul_pairing(out, x, interleaved ? 1 : 0); }

void gelu_tanh(torch::Tensor out, torch::Tensor x) {
  dev_bf16(out, "out"); dev_bf16(x, "x");
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous() && x.numel() == out.numel(), "gelu: shape");
  check(k8sllm_gelu_tanh(out.data_ptr(), x.data_ptr(), x.numel(), cur()), "gelu_tanh");
}

void embedding(torch::Tensor out, torch::Tensor ids, torch::Tensor weight, int64_t vocab_start) {
  dev_bf16(out, "out"); dev_bf16(weight, "weight"); dev_i32(ids, "ids");
  TORCH_CHECK(weight.is_contiguous() && out.is_contiguous(), "embedding: contiguous");
  const int d = (int)weight.size(1);
  check(k8sllm_embedding(out.data_ptr(), ids.data_ptr<int>(), weight.data_ptr(), ids.numel(), d, (int)vocab_start,
                         (int)weight.size(0), cur()),
        "embedding");
}

void resolve_ids(torch::Tensor out, torch::Tensor ids, torch::Tensor src, torch::Tensor prev) {
  dev_i32(out, "out"); dev_i32(ids, "ids"); dev_i32(src, "src"); dev_i32(prev, "prev");
  TORCH_CHECK(out.is_contiguous() && ids.is_contiguous() && src.is_contiguous() && prev.is_contiguous(),
              "resolve_ids: contiguous");
  TORCH_CHECK(ids.numel() == out.numel() && src.numel() == out.numel(), "resolve_ids: sizes");
  check(k8sllm_resolve_ids(out.data_ptr<int>(), ids.data_ptr<int>(), src.data_ptr<int>(), prev.data_ptr<int>(),
                           (int)out.numel(), cur()),
        "resolve_ids");
}

void rope_and_cache(torch::Tensor qkv, torch::Tensor positions, torch::Tensor cos_sin, torch::Tensor k_cache,
                    torch::Tensor v_cache, torch::Tensor slot_mapping, int64_t Hq, int64_t Hkv, int64_t D,
                    bool apply_rope, c10::optional<torch::Tensor> partial, int64_t S,
                    c10::optional<torch::Tensor> kv_scale, c10::optional<torch::Tensor> q_norm_w,
                    c10::optional<torch::Tensor> k_norm_w, double eps) {
  dev_bf16(qkv, "qkv"); dev_i32(positions, "positions");
  // QK-norm: one [D] weight for every q head and one for every k head, both fp32 or both bf16
  TORCH_CHECK(q_norm_w.has_value() == k_norm_w.has_value(), "qk_norm: q and k weights come together");
  const void *qnw = nullptr, *knw = nullptr;
  int norm_bf16 = 0;
  if (q_norm_w.has_value()) {
    const torch::Tensor &qw = *q_norm_w, &kw = *k_norm_w;
    TORCH_CHECK(qw.is_cuda() && kw.is_cuda() && qw.device() == qkv.device() && kw.device() == qkv.device(),
                "qk_norm: weights must be on qkv's device");
    TORCH_CHECK(qw.scalar_type() == kw.scalar_type() &&
                    (qw.scalar_type() == torch::kFloat32 || qw.scalar_type() == torch::kBFloat16),
                "qk_norm: weights must both be fp32 or both bf16");
    TORCH_CHECK(qw.dim() == 1 && kw.dim() == 1 && qw.size(0) == D && kw.size(0) == D && qw.is_contiguous() &&
                    kw.is_contiguous(),
                "qk_norm: weights must be contiguous [D]");
    TORCH_CHECK(std::isfinite(eps) && eps >= 0.0, "qk_norm: eps must be finite and >= 0");
    qnw = qw.data_ptr();
    knw = kw.data_ptr();
    norm_bf16 = qw.scalar_type() == torch::kBFloat16 ? 1 : 0;
  }
  TORCH_CHECK(qkv.stride(-1) == 1 && qkv.dim() == 2, "qkv must be [T, (Hq+2Hkv)*D] with unit inner stride");
  TORCH_CHECK(qkv.size(1) >= (Hq + 2 * Hkv) * D, "qkv width");
  TORCH_CHECK(cos_sin.scalar_type() == torch::kFloat32 && cos_sin.is_contiguous() && cos_sin.size(1) == D, "cos_sin");
  const bool has_cache = slot_mapping.numel() > 0;
  int block_size = 16;
  float* ksp = nullptr;
  if (has_cache) {
    dev_i32(slot_mapping, "slot_mapping");
    ksp = kv_cache_pair(k_cache, v_cache, kv_scale, Hkv, D);
    // k_cache [NB, Hkv, D/8, BS, 8], v_cache [NB, Hkv, D, BS]
    TORCH_CHECK(k_cache.dim() == 5 && k_cache.size(1) == Hkv && k_cache.size(4) == 8, "k_cache layout");
    TORCH_CHECK(v_cache.dim() == 4 && v_cache.size(1) == Hkv && v_cache.size(2) == D, "v_cache layout");
    block_size = (int)k_cache.size(3);
  }
  const float* pp = nullptr;
  if (partial.has_value()) {  // qkv = sum of S fp32 split-K slabs [S][T][(Hq+2Hkv)*D]
    TORCH_CHECK(partial->is_cuda() && partial->scalar_type() == torch::kFloat32 && partial->is_contiguous(), "partial");
    TORCH_CHECK(partial->numel() >= S * qkv.size(0) * (Hq + 2 * Hkv) * D, "partial too small");
    pp = partial->data_ptr<float>();
  }
  check(k8sllm_rope_cache(qkv.data_ptr(), qkv.stride(0), positions.data_ptr<int>(), cos_sin.data_ptr<float>(),
                          has_cache ? k_cache.data_ptr() : nullptr, has_cache ? v_cache.data_ptr() : nullptr,
                          has_cache ? slot_mapping.data_ptr<int>() : nullptr, qkv.size(0), (int)Hq, (int)Hkv, (int)D,
                          block_size, apply_rope ? 1 : 0, pp, (int)S, ksp, qnw, knw, (float)eps, norm_bf16, cur()),
        "rope_and_cache");
}

// What paged_decode and paged_decode_fused check alike.  Every rule about numbers - the head dim,
// the query heads per KV head, the split range, the fp8 head dim - is pd_plan's
// (paged_decode_forms.h); here: the tensors' layouts, dtypes and sizes.  Returns (the scales'
// pointer or null, the launcher's out_stride, B).
struct PdArgs {
  float* kv_scale;
  long out_stride;
  int B;
};

PdArgs pd_check(const char* what, bool fused, const torch::Tensor& out, const torch::Tensor& k_cache,
                const torch::Tensor& v_cache, const c10::optional<torch::Tensor>& kv_scale,
                const torch::Tensor& block_tables, const torch::Tensor& seq_lens, const torch::Tensor& part_out,
                const torch::Tensor& part_ml, int64_t Hq, int64_t Hkv, int64_t D, int64_t splits) {
  dev_bf16(out, "out");
  dev_i32(block_tables, "block_tables"); dev_i32(seq_lens, "seq_lens");
  const int B = (int)seq_lens.size(0);
  const bool f8 = k_cache.scalar_type() == torch::kFloat8_e4m3fn;
  const k8sllm::PdPlan p = k8sllm::pd_plan((int)D, (int)Hq, (int)Hkv, B, (int)splits, fused, f8, false, 0);
  TORCH_CHECK(p.err != -2, what, ": splits must be in [1, ", k8sllm::kPdMaxSplits, "]");
  TORCH_CHECK(p.err != -3, what, ": ", fused ? "the fused form" : "an fp8 KV cache", " needs head_dim 128, not ", D);
  TORCH_CHECK(p.err == 0, what, ": no ", fused ? "fused " : "", f8 ? "fp8" : "bf16", " form for head_dim ", D, " with ",
              Hq, " query heads over ", Hkv, " KV heads");
  float* ksp = kv_cache_pair(k_cache, v_cache, kv_scale, Hkv, D);
  const bool packed = out.dim() == 4;  // fragment-packed [ceil(B/16), Hq*D/32, 64, 8] for gemm_skinny
  if (packed) {
    TORCH_CHECK(out.is_contiguous() && out.size(1) * 32 == Hq * D && out.size(2) == 64 && out.size(3) == 8 &&
                    out.size(0) * 16 >= B, "packed out must be [ceil(B/16), Hq*D/32, 64, 8]");
  } else {
    TORCH_CHECK(out.dim() == 2 && out.stride(1) == 1 && out.size(1) == Hq * D, "out must be [B, Hq*D]");
  }
  TORCH_CHECK(k_cache.dim() == 5 && v_cache.dim() == 4 && k_cache.size(1) == Hkv && k_cache.size(3) == k8sllm::kBS &&
                  v_cache.size(3) == k8sllm::kBS,
              what, " expects block_size 16: caches [NB, Hkv, D/8, 16, 8] / [NB, Hkv, D, 16]");
  TORCH_CHECK(part_out.scalar_type() == torch::kFloat32 && part_ml.scalar_type() == torch::kFloat32, "partials fp32");
  TORCH_CHECK(part_out.numel() >= (int64_t)B * Hq * splits * D && part_ml.numel() >= (int64_t)B * Hq * splits * 2,
              "decode workspace too small for batch x splits");
  return {ksp, packed ? -(long)(Hq * D / 32) : (long)out.stride(0), B};
}

void paged_decode(torch::Tensor out, torch::Tensor q, torch::Tensor k_cache, torch::Tensor v_cache,
                  torch::Tensor block_tables, torch::Tensor seq_lens, torch::Tensor part_out, torch::Tensor part_ml,
                  int64_t Hq, int64_t Hkv, int64_t D, double scale, int64_t splits,
                  c10::optional<torch::Tensor> kv_scale) {
  const PdArgs a = pd_check("paged_decode", false, out, k_cache, v_cache, kv_scale, block_tables, seq_lens, part_out,
                            part_ml, Hq, Hkv, D, splits);
  dev_bf16(q, "q");
  TORCH_CHECK(q.dim() == 2 && q.stride(1) == 1, "q must be [B, >=Hq*D] rows");
  check(k8sllm_paged_decode(out.data_ptr(), a.out_stride, part_out.data_ptr<float>(), part_ml.data_ptr<float>(),
                            q.data_ptr(), q.stride(0), k_cache.data_ptr(), v_cache.data_ptr(),
                            block_tables.data_ptr<int>(), (int)block_tables.stride(0), seq_lens.data_ptr<int>(), a.B,
                            (int)Hq, (int)Hkv, (int)D, (int)splits, (float)scale, a.kv_scale, nullptr, 0, nullptr,
                            nullptr, nullptr, nullptr, cur()),
        "paged_decode");
}

// paged_decode with the new token's q / k / v taken from the qkv projection's fp32 split-K slabs
// [nslabs, B, (Hq + 2 Hkv) * D] (summed, rounded, RoPE at positions, k / v written to the cache at
// slot_mapping inside the attention kernel: rope_and_cache folded in).  D = 128.
void paged_decode_fused(torch::Tensor out, torch::Tensor slabs, int64_t nslabs, torch::Tensor positions,
                        torch::Tensor cos_sin, torch::Tensor slot_mapping, torch::Tensor k_cache,
                        torch::Tensor v_cache, torch::Tensor block_tables, torch::Tensor seq_lens,
                        torch::Tensor part_out, torch::Tensor part_ml, int64_t Hq, int64_t Hkv, int64_t D,
                        double scale, int64_t splits, torch::Tensor merge_ctr,
                        c10::optional<torch::Tensor> kv_scale) {
  const PdArgs a = pd_check("paged_decode_fused", true, out, k_cache, v_cache, kv_scale, block_tables, seq_lens,
                            part_out, part_ml, Hq, Hkv, D, splits);
  const int B = a.B;
  dev_i32(positions, "positions");
  TORCH_CHECK(slabs.is_cuda() && slabs.scalar_type() == torch::kFloat32 && slabs.is_contiguous() &&
                  slabs.numel() >= nslabs * B * (Hq + 2 * Hkv) * D && nslabs >= 1,
              "paged_decode_fused: slabs must hold nslabs x [B, (Hq + 2 Hkv) * D] fp32");
  TORCH_CHECK(positions.numel() >= B, "paged_decode_fused: positions [B]");
  TORCH_CHECK(cos_sin.is_cuda() && cos_sin.scalar_type() == torch::kFloat32 && cos_sin.is_contiguous() &&
                  cos_sin.size(1) == D, "paged_decode_fused: cos_sin [max_pos, D] fp32");
  const bool has_slots = slot_mapping.numel() > 0;
  if (has_slots) {
    dev_i32(slot_mapping, "slot_mapping");
    TORCH_CHECK(slot_mapping.numel() >= B, "paged_decode_fused: slot_mapping [B]");
  }
  // merge_ctr (numel > 0): B x Hkv int32 counters, zero between launches (the kernel resets them)
  const bool merge = merge_ctr.numel() > 0;
  if (merge) {
    dev_i32(merge_ctr, "merge_ctr");
    TORCH_CHECK(merge_ctr.numel() >= (int64_t)B * Hkv, "paged_decode_fused: merge_ctr must hold B x Hkv counters");
  }
  check(k8sllm_paged_decode(out.data_ptr(), a.out_stride, part_out.data_ptr<float>(), part_ml.data_ptr<float>(),
                            nullptr, 0, k_cache.data_ptr(), v_cache.data_ptr(), block_tables.data_ptr<int>(),
                            (int)block_tables.stride(0), seq_lens.data_ptr<int>(), B, (int)Hq, (int)Hkv, (int)D,
                            (int)splits, (float)scale, a.kv_scale, slabs.data_ptr<float>(), (int)nslabs,
                            positions.data_ptr<int>(), cos_sin.data_ptr<float>(),
                            has_slots ? slot_mapping.data_ptr<int>() : nullptr,
                            merge ? merge_ctr.data_ptr<int>() : nullptr, cur()),
        "paged_decode_fused");
}

// pd_plan (paged_decode_forms.h), what a launch with these arguments does: (err, row of
// paged_decode_forms(), TW, merge, reduce, grid x, y, z).  tw_force: what decode_tw_force was given.
// No launch.
std::vector<int64_t> paged_decode_plan(int64_t D, int64_t Hq, int64_t Hkv, int64_t B, int64_t S, bool fused, bool f8,
                                       bool merge_wanted, int64_t tw_force) {
  const k8sllm::PdPlan p =
      k8sllm::pd_plan((int)D, (int)Hq, (int)Hkv, (int)B, (int)S, fused, f8, merge_wanted, (int)tw_force);
  return {p.err, p.form, p.tw, p.merge, p.reduce, p.gx, p.gy, p.gz};
}

// The compiled forms of paged decode (kPdForms): (D, G, fused, fp8 cache) per row.
std::vector<std::vector<int64_t>> paged_decode_forms() {
  std::vector<int> v(4 * k8sllm::kPdNForms);
  const int n = k8sllm_paged_decode_forms(v.data(), k8sllm::kPdNForms);
  TORCH_CHECK(n == k8sllm::kPdNForms, "paged_decode_forms: ", n, " rows compiled, ", k8sllm::kPdNForms, " in the header");
  std::vector<std::vector<int64_t>> rows;
  for (int i = 0; i < n; ++i) rows.emplace_back(v.begin() + 4 * i, v.begin() + 4 * i + 4);
  return rows;
}

// paged (optional, all or none): ctx_start [S] (cached tokens before each sequence's new rows),
// k_cache / v_cache (already holding the new tokens), block_tables [S, W] -> attention over the
// whole context from the paged cache (prefix caching / chunked prefill).
void flash_prefill(torch::Tensor out, torch::Tensor qkv, torch::Tensor cu_seqlens, torch::Tensor qb_seq,
                   torch::Tensor qb_start, int64_t Hq, int64_t Hkv, int64_t D, double scale,
                   c10::optional<torch::Tensor> ctx_start, c10::optional<torch::Tensor> k_cache,
                   c10::optional<torch::Tensor> v_cache, c10::optional<torch::Tensor> block_tables,
                   c10::optional<torch::Tensor> kv_scale) {
  dev_bf16(out, "out"); dev_bf16(qkv, "qkv");
  dev_i32(cu_seqlens, "cu_seqlens"); dev_i32(qb_seq, "qb_seq"); dev_i32(qb_start, "qb_start");
  TORCH_CHECK(qkv.dim() == 2 && qkv.stride(1) == 1, "qkv rows");
  TORCH_CHECK(out.dim() == 2 && out.stride(1) == 1 && out.size(1) == Hq * D, "out must be [T, Hq*D]");
  const int* cs = nullptr;
  const void *kc = nullptr, *vc = nullptr;
  const int* bt = nullptr;
  const float* ksp = nullptr;
  int bts = 0;
  if (ctx_start.has_value()) {
    TORCH_CHECK(k_cache.has_value() && v_cache.has_value() && block_tables.has_value(), "paged prefill needs caches");
    dev_i32(*ctx_start, "ctx_start"); dev_i32(*block_tables, "block_tables");
    ksp = kv_cache_pair(*k_cache, *v_cache, kv_scale, Hkv, D);
    TORCH_CHECK(k_cache->dim() == 5 && k_cache->size(1) == Hkv && k_cache->size(3) == 16 && k_cache->size(4) == 8,
                "k_cache layout [NB, Hkv, D/8, 16, 8]");
    TORCH_CHECK(v_cache->dim() == 4 && v_cache->size(1) == Hkv && v_cache->size(2) == D && v_cache->size(3) == 16,
                "v_cache layout [NB, Hkv, D, 16]");
    TORCH_CHECK(block_tables->dim() == 2 && block_tables->size(0) == cu_seqlens.numel() - 1, "block_tables [S, W]");
    cs = ctx_start->data_ptr<int>();
    kc = k_cache->data_ptr();
    vc = v_cache->data_ptr();
    bt = block_tables->data_ptr<int>();
    bts = (int)block_tables->stride(0);
  }
  check(k8sllm_flash_prefill(out.data_ptr(), out.stride(0), qkv.data_ptr(), qkv.stride(0), cu_seqlens.data_ptr<int>(),
                             qb_seq.data_ptr<int>(), qb_start.data_ptr<int>(), (int)qb_seq.numel(), (int)Hq, (int)Hkv,
                             (int)D, (float)scale, cs, kc, vc, bt, bts, ksp, cur()),
        "flash_prefill");
}

static void check_penalty_state(const torch::Tensor& table, const torch::Tensor& params, int64_t vocab) {
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kInt16 && table.dim() == 2 && table.is_contiguous() &&
                  table.size(1) % 8 == 0 && vocab > 0 && vocab <= table.size(1),
              "penalty table: contiguous int16 [slots, stride], stride a multiple of 8 and >= the vocabulary");
  TORCH_CHECK(params.is_cuda() && params.scalar_type() == torch::kFloat32 && params.is_contiguous() &&
                  params.dim() == 2 && params.size(0) == table.size(0) && params.size(1) == 4,
              "penalty params: contiguous fp32 [slots, 4]");
}

static void check_guide_state(const torch::Tensor& mask, const torch::Tensor& trans, const torch::Tensor& tok_off,
                              const torch::Tensor& blob, const torch::Tensor& eos, int64_t vocab) {
  TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == torch::kInt32 && mask.dim() == 2 && mask.is_contiguous() &&
                  mask.size(1) % 4 == 0 && vocab > 0 && vocab <= mask.size(1) * 32,
              "guide mask: contiguous int32 [rows, W], W a multiple of 4 words covering the vocabulary");
  TORCH_CHECK(trans.is_cuda() && trans.scalar_type() == torch::kInt32 && trans.is_contiguous() && trans.dim() == 2 &&
                  trans.size(0) == mask.size(0) && trans.size(1) == 256,
              "guide trans: contiguous int32 [rows, 256]");
  TORCH_CHECK(tok_off.is_cuda() && tok_off.scalar_type() == torch::kInt32 && tok_off.is_contiguous() &&
                  tok_off.numel() == vocab + 1,
              "guide tok_off: contiguous int32 [V + 1]");
  TORCH_CHECK(blob.is_cuda() && blob.scalar_type() == torch::kUInt8 && blob.is_contiguous(), "guide blob: uint8");
  TORCH_CHECK(eos.is_cuda() && eos.scalar_type() == torch::kInt32 && eos.is_contiguous(), "guide eos: int32");
}

void sample(torch::Tensor out, torch::Tensor logits, c10::optional<torch::Tensor> temps,
            c10::optional<torch::Tensor> top_k, c10::optional<torch::Tensor> top_p, c10::optional<torch::Tensor> rng,
            bool advance, c10::optional<torch::Tensor> pen_table, c10::optional<torch::Tensor> pen_params,
            c10::optional<torch::Tensor> pen_slots, int64_t pen_vocab, c10::optional<torch::Tensor> g_mask,
            c10::optional<torch::Tensor> g_trans, c10::optional<torch::Tensor> g_state,
            c10::optional<torch::Tensor> g_slots, c10::optional<torch::Tensor> g_tok_off,
            c10::optional<torch::Tensor> g_blob, c10::optional<torch::Tensor> g_eos) {
  dev_i32(out, "out");
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1, "logits [B, V]");
  const bool f32 = logits.scalar_type() == torch::kFloat32;
  TORCH_CHECK(f32 || logits.scalar_type() == torch::kBFloat16, "logits must be fp32 or bf16");
  const float* t = temps && temps->numel() ? temps->data_ptr<float>() : nullptr;
  const int* k = top_k && top_k->numel() ? top_k->data_ptr<int>() : nullptr;
  const float* p = top_p && top_p->numel() ? top_p->data_ptr<float>() : nullptr;
  const int64_t* r = rng && rng->numel() ? rng->data_ptr<int64_t>() : nullptr;
  const long B = logits.size(0);
  const int V = (int)logits.size(1);
  const int64_t np = B * k8sllm_sample_parts(B, V);
  // partial (value, index) workspace: stream-ordered caching allocator (graph-pool safe)
  auto pv = torch::empty({np}, logits.options().dtype(torch::kFloat32));
  auto pi = torch::empty({np}, logits.options().dtype(torch::kInt32));
  // penalty state (ops.PenaltyState): table [slots, stride] int16, params [slots, 4] fp32, slots [B] int32
  const int* ps = nullptr;
  void* tb = nullptr;
  const float* pp = nullptr;
  long tstride = 0;
  int nslots = 0;
  if (pen_table) {
    TORCH_CHECK(pen_params && pen_slots, "sample: penalties need params and slots");
    check_penalty_state(*pen_table, *pen_params, pen_vocab);
    TORCH_CHECK(pen_vocab == V, "sample: the penalty state is for a vocabulary of ", pen_vocab, ", logits have ", V);
    dev_i32(*pen_slots, "slots");
    TORCH_CHECK(pen_slots->is_contiguous() && pen_slots->numel() >= B, "sample: slots [B]");
    ps = pen_slots->data_ptr<int>();
    tb = pen_table->data_ptr();
    pp = pen_params->data_ptr<float>();
    tstride = pen_table->size(1);
    nslots = (int)pen_table->size(0);
  }
  // guide state (ops.GuideState): mask [rows, W] / trans [rows, 256] / state [slots] / slots [B] int32,
  // the vocabulary as CSR (tok_off int32 [V + 1], blob uint8) and the eos ids int32
  const int *gs = nullptr, *gt = nullptr, *go = nullptr, *ge = nullptr;
  int* gst = nullptr;
  const void *gm = nullptr, *gb = nullptr;
  int gW = 0, grows = 0, gnslots = 0, n_eos = 0;
  if (g_mask) {
    TORCH_CHECK(g_trans && g_state && g_slots && g_tok_off && g_blob && g_eos,
                "sample: a guide needs trans, state, slots, tok_off, blob and eos");
    check_guide_state(*g_mask, *g_trans, *g_tok_off, *g_blob, *g_eos, V);
    dev_i32(*g_state, "guide state"); dev_i32(*g_slots, "guide slots");
    TORCH_CHECK(g_state->is_contiguous() && g_state->numel() > 0, "sample: guide state [slots]");
    TORCH_CHECK(g_slots->is_contiguous() && g_slots->numel() >= B, "sample: guide slots [B]");
    gm = g_mask->data_ptr();
    gW = (int)g_mask->size(1);
    grows = (int)g_mask->size(0);
    gt = g_trans->data_ptr<int>();
    gst = g_state->data_ptr<int>();
    gnslots = (int)g_state->numel();
    gs = g_slots->data_ptr<int>();
    go = g_tok_off->data_ptr<int>();
    gb = g_blob->data_ptr();
    n_eos = (int)g_eos->numel();
    ge = n_eos ? g_eos->data_ptr<int>() : nullptr;
  }
  check(k8sllm_sample_guided(out.data_ptr<int>(), logits.data_ptr(), f32 ? 1 : 0, B, logits.stride(0), V, t, k, p, r,
                             pv.data_ptr<float>(), pi.data_ptr<int>(), advance ? 1 : 0, ps, tb, tstride, pp, nslots,
                             gs, gst, gnslots, gm, gW, gt, grows, go, gb, ge, n_eos, cur()),
        "sample");
}

// Fill the mask rows of one guide (ops.GuideState.load): rows int32 [n] (device) are its absolute rows
void guide_mask_build(torch::Tensor mask, torch::Tensor trans, torch::Tensor accept, torch::Tensor popc,
                      torch::Tensor rows, torch::Tensor tok_off, torch::Tensor blob, torch::Tensor eos) {
  const int64_t V = tok_off.numel() - 1;
  check_guide_state(mask, trans, tok_off, blob, eos, V);
  dev_i32(popc, "popc"); dev_i32(rows, "rows");
  TORCH_CHECK(accept.is_cuda() && accept.scalar_type() == torch::kUInt8 && accept.is_contiguous() &&
                  accept.numel() == mask.size(0),
              "guide accept: uint8 [rows]");
  TORCH_CHECK(popc.is_contiguous() && popc.numel() == mask.size(0), "guide popc: int32 [rows]");
  TORCH_CHECK(rows.is_contiguous() && rows.numel() <= mask.size(0), "guide rows: int32 [n]");
  check(k8sllm_guide_mask_build(mask.data_ptr(), (int)mask.size(1), trans.data_ptr<int>(), accept.data_ptr(),
                                popc.data_ptr<int>(), rows.data_ptr<int>(), (int)rows.numel(), (int)mask.size(0),
                                tok_off.data_ptr<int>(), blob.data_ptr(), (int)V,
                                eos.numel() ? eos.data_ptr<int>() : nullptr, (int)eos.numel(), cur()),
        "guide_mask_build");
}

void penalty_reset(torch::Tensor table, torch::Tensor params, int64_t vocab, int64_t slot, torch::Tensor ids,
                   int64_t n_prompt, int64_t n_out, double rep, double inv_rep, double presence, double frequency) {
  check_penalty_state(table, params, vocab);
  dev_i32(ids, "ids");
  TORCH_CHECK(slot >= 0 && slot < table.size(0), "penalty_reset: slot ", slot, " of ", table.size(0));
  TORCH_CHECK(ids.is_contiguous() && n_prompt >= 0 && n_out >= 0 && n_prompt + n_out <= ids.numel(),
              "penalty_reset: ids holds n_prompt + n_out entries");
  check(k8sllm_penalty_reset(table.data_ptr(), table.size(1), (int)vocab, (int)table.size(0), (int)slot,
                             ids.data_ptr<int>(), (int)n_prompt, (int)n_out, params.data_ptr<float>(), (float)rep,
                             (float)inv_rep, (float)presence, (float)frequency, cur()),
        "penalty_reset");
}

// Last-token pooling (ops.pool_l2): x bf16 / fp32 [R, d] (rows may be strided), dim int32 [>= R], out fp32 [R, d]
void pool_l2(torch::Tensor out, torch::Tensor x, torch::Tensor dim) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.stride(1) == 1 && x.stride(0) >= x.size(1),
              "pool_l2: x must be a 2-D GPU tensor with unit column stride");
  const bool f32 = x.scalar_type() == torch::kFloat32;
  TORCH_CHECK(f32 || x.scalar_type() == torch::kBFloat16, "pool_l2: x must be bfloat16 or float32");
  const long R = x.size(0);
  const int d = (int)x.size(1);
  dev_i32(dim, "dim");
  TORCH_CHECK(dim.numel() >= R, "pool_l2: dim [R]");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kFloat32 && out.is_contiguous() && out.dim() == 2 &&
                  out.size(0) == R && out.size(1) == d,
              "pool_l2: out must be contiguous float32 [R, d]");
  if (R == 0) return;
  check(k8sllm_pool_l2(out.data_ptr<float>(), x.data_ptr(), f32 ? 1 : 0, dim.data_ptr<int>(), R, d, x.stride(0),
                       cur()),
        "pool_l2");
}

// Token log-probabilities (ops.token_logprobs): out int32 [>= B, 41] packed records, tok / want int32 [>= B]
void token_logprobs(torch::Tensor out, torch::Tensor logits, torch::Tensor tok, torch::Tensor want) {
  dev_i32(out, "out"); dev_i32(tok, "tok"); dev_i32(want, "want");
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1, "logits [B, V]");
  const bool f32 = logits.scalar_type() == torch::kFloat32;
  TORCH_CHECK(f32 || logits.scalar_type() == torch::kBFloat16, "logits must be fp32 or bf16");
  const long B = logits.size(0);
  const int V = (int)logits.size(1);
  TORCH_CHECK(V > 0, "token_logprobs: empty vocabulary");
  TORCH_CHECK(tok.numel() >= B && want.numel() >= B, "token_logprobs: tok [B], want [B]");
  TORCH_CHECK(out.dim() == 2 && out.size(0) >= B && out.size(1) == 41, "token_logprobs: out int32 [>= B, 41]");
  if (B == 0) return;
  // partials and candidates: stream-ordered caching allocator (graph-pool safe), like sample
  auto ws = torch::empty({(int64_t)k8sllm_token_logprobs_ws(B, V)}, logits.options().dtype(torch::kInt32));
  check(k8sllm_token_logprobs(out.data_ptr<int>(), logits.data_ptr(), f32 ? 1 : 0, B, logits.stride(0), V,
                              tok.data_ptr<int>(), want.data_ptr<int>(), ws.data_ptr(), cur()),
        "token_logprobs");
}

void moe_router(torch::Tensor x, torch::Tensor wr, torch::Tensor ids, torch::Tensor w, torch::Tensor wd, bool renorm) {
  dev_bf16(x, "x"); dev_bf16(wr, "router"); dev_i32(ids, "ids");
  TORCH_CHECK(x.is_contiguous() && x.dim() == 2 && wr.is_contiguous() && wr.dim() == 2 && wr.size(1) == x.size(1),
              "moe_router: x [T, d], router [E, d]");
  const long T = x.size(0);
  const int E = (int)wr.size(0), K = (int)ids.size(1);
  TORCH_CHECK(ids.dim() == 2 && ids.size(0) == T && w.is_cuda() && w.scalar_type() == torch::kFloat32 &&
                  w.sizes() == ids.sizes() && wd.is_cuda() && wd.scalar_type() == torch::kFloat32 &&
                  wd.is_contiguous() && wd.numel() == T * E, "moe_router: ids / w [T, K], wd [T, E] fp32");
  check(k8sllm_moe_router(x.data_ptr(), wr.data_ptr(), T, (int)x.size(1), E, K, renorm ? 1 : 0, ids.data_ptr<int>(),
                          w.data_ptr<float>(), wd.data_ptr<float>(), cur()),
        "moe_router");
}

void moe_route(torch::Tensor logits, torch::Tensor topk_ids, torch::Tensor topk_w, bool renorm) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous(), "router logits");
  TORCH_CHECK(logits.scalar_type() == torch::kFloat32, "router logits must be fp32");
  dev_i32(topk_ids, "topk_ids");
  const int E = (int)logits.size(1);
  const int K = (int)topk_ids.size(1);
  TORCH_CHECK(E <= 64 && K <= E, "moe_route supports up to 64 experts");
  check(k8sllm_moe_route(logits.data_ptr(), logits.size(0), E, K, renorm ? 1 : 0, topk_ids.data_ptr<int>(),
                         topk_w.data_ptr<float>(), cur()),
        "moe_route");
}

void moe_align(torch::Tensor topk_ids, int64_t E, torch::Tensor expert_offsets, torch::Tensor sorted_idx,
               torch::Tensor inv_idx) {
  dev_i32(topk_ids, "topk_ids"); dev_i32(expert_offsets, "expert_offsets");
  dev_i32(sorted_idx, "sorted_idx"); dev_i32(inv_idx, "inv_idx");
  TORCH_CHECK(expert_offsets.numel() == E + 1, "expert_offsets size");
  check(k8sllm_moe_align(topk_ids.data_ptr<int>(), topk_ids.numel(), (int)E, expert_offsets.data_ptr<int>(),
                         sorted_idx.data_ptr<int>(), inv_idx.data_ptr<int>(), cur()),
        "moe_align");
}

void moe_combine(torch::Tensor out, torch::Tensor expert_out, torch::Tensor inv_idx, torch::Tensor topk_w) {
  dev_bf16(out, "out"); dev_bf16(expert_out, "expert_out"); dev_i32(inv_idx, "inv_idx");
  TORCH_CHECK(out.is_contiguous() && expert_out.is_contiguous(), "moe_combine contiguous");
  const int d = (int)out.size(1);
  check(k8sllm_moe_combine(out.data_ptr(), expert_out.data_ptr(), inv_idx.data_ptr<int>(), topk_w.data_ptr<float>(),
                           out.size(0), (int)topk_w.size(1), d, cur()),
        "moe_combine");
}

// Grouped expert GEMM over expert-sorted rows (moe_gemm.hip): x [rows, K], w [E, N, K], offsets
// [E + 1] int32 absolute row offsets of the experts in x (device, from moe_align; no host sync).
// swiglu: w gate/up-interleaved per 128 rows, y [rows, N / 2] = silu(gate) * up; else y [rows, N].
// Rows outside [offsets[0], offsets[E]) are not written.
void moe_grouped_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor w, torch::Tensor offsets, bool swiglu) {
  dev_bf16(y, "y"); dev_bf16(x, "x"); dev_bf16(w, "w"); dev_i32(offsets, "offsets");
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous() && w.dim() == 3 && w.is_contiguous() && y.is_contiguous(),
              "moe_grouped_gemm: x [rows, K], w [E, N, K] contiguous");
  const int E = (int)w.size(0), N = (int)w.size(1), K = (int)w.size(2);
  TORCH_CHECK(x.size(1) == K, "moe_grouped_gemm: K mismatch");
  TORCH_CHECK(offsets.numel() == E + 1, "moe_grouped_gemm: offsets must hold E + 1 entries");
  TORCH_CHECK(N % 128 == 0 && K % 64 == 0, "moe_grouped_gemm: N % 128 == 0 and K % 64 == 0");
  TORCH_CHECK(y.size(0) == x.size(0) && y.size(1) == (swiglu ? N / 2 : N), "moe_grouped_gemm: y shape");
  check(k8sllm_moe_grouped_gemm(x.data_ptr(), w.data_ptr(), y.data_ptr(), offsets.data_ptr<int>(), E, x.size(0), N, K,
                                (long)N * K, swiglu ? 1 : 0, cur()),
        "moe_grouped_gemm");
}

// 256 x 256 MFMA GEMM (gemm_tile.hip) for prefill-sized projections: y = x . w^T, x [M, K], w [N, K]
// (dense, offsets None) or w [E, N, K] with device offsets [E + 1] (grouped over expert-sorted rows,
// no host sync), row-major or fragment-packed [N/16, K/32, 64, 8] (pack_skinny); or the tensors
// gemm_dec streams: fp8 codes [N/16, K/64, 64, 16] + wscale [N] fp32 (pack_skinny_f8), mxfp4 codes
// [N/16, K/128, 64, 16] uint8 + wscale [N/16, K/128, 16, 4] uint8 (pack_skinny_f4).
// swiglu: 0 none, 1 = gate/up interleaved per 128 rows (interleave_gate_up), 8 = per 16 rows
// (interleave_gate_up8); rope_pos / rope_cs: RoPE of heads 0 .. rope_heads - 1 (head_dim 128) in the
// epilogue; rs_part: the deferred RMSNorm row scale; resid / hw / norm_w / ss_out: the residual epilogue.
// Which combinations are compiled and every limit on M, N, K, E and the schedule: tile_plan
// (gemm_tile_forms.h).  Here: the tensors' layouts, dtypes, devices and sizes.
// persist / cus (A/B runs; tile_plan): -1 = the persistent form where the table routes the launch,
// 1 = wherever it is compiled, 0 = nowhere; cus: the persistent grid's size, 0 = the device's CUs.
void gemm_tile(torch::Tensor y, torch::Tensor x, torch::Tensor w, c10::optional<torch::Tensor> offsets, int64_t swiglu,
               int64_t algo, c10::optional<torch::Tensor> rope_pos, c10::optional<torch::Tensor> rope_cs,
               int64_t rope_heads, c10::optional<torch::Tensor> rs_part, double rs_eps,
               c10::optional<torch::Tensor> resid, c10::optional<torch::Tensor> hw,
               c10::optional<torch::Tensor> norm_w, c10::optional<torch::Tensor> ss_out,
               c10::optional<torch::Tensor> wscale, int64_t persist, int64_t cus) {
  using namespace k8sllm;
  dev_bf16(y, "y"); dev_bf16(x, "x");
  TORCH_CHECK(persist >= -1 && persist <= 1 && cus >= 0 && cus <= (1 << 20), "gemm_tile: persist -1, 0 or 1; cus >= 0");
  const int fmt = w.scalar_type() == torch::kFloat8_e4m3fn ? TILE_W_F8 : w.scalar_type() == torch::kUInt8 ? TILE_W_F4 : TILE_W_BF16;
  const bool quant = fmt != TILE_W_BF16;
  const std::string whats = std::string("gemm_tile (") + (fmt == TILE_W_F4 ? "mxfp4)" : fmt == TILE_W_F8 ? "fp8)" : "bf16)");
  const char* what = whats.c_str();
  if (quant) {
    TORCH_CHECK(w.is_cuda(), "w must be a GPU tensor");
  } else {
    dev_bf16(w, "w");
  }
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous() && w.is_contiguous() && y.is_contiguous(),
              "gemm_tile: x [M, K], w contiguous, y contiguous");
  const bool grouped = offsets.has_value();
  const int g = grouped ? 1 : 0;
  const bool wpk = w.dim() == 4 + g;  // fragment-packed blocks (codes always are), else row-major
  TORCH_CHECK(wpk ? w.size(-2) == 64 && w.size(-1) == (quant ? 16 : 8) : !quant && w.dim() == 2 + g, what,
              ": w must be bf16 [N, K] or fragment-packed [N/16, K/32, 64, 8], float8_e4m3fn [N/16, K/64, 64, 16] "
              "or uint8 [N/16, K/128, 64, 16], or an [E, ...] stack of such with offsets");
  const int E = grouped ? (int)w.size(0) : 1;
  const int N = wpk ? (int)w.size(g) * 16 : (int)w.size(g);
  const int K = wpk ? (int)w.size(g + 1) * (fmt == TILE_W_F4 ? 128 : fmt == TILE_W_F8 ? 64 : 32) : (int)w.size(g + 1);
  const int M = (int)x.size(0);
  TORCH_CHECK(x.size(1) == K, "gemm_tile: K mismatch");
  TORCH_CHECK(swiglu == 0 || swiglu == 1 || swiglu == 8, "gemm_tile: swiglu 0, 1 or 8");
  const bool rsd = resid.has_value(), rp = rope_pos.has_value(), rs = rs_part.has_value();
  TORCH_CHECK(!(rp && swiglu) && !(rsd && (swiglu || rp)), "gemm_tile: one epilogue - swiglu, rope or the residual one");
  TORCH_CHECK(!rs || K % 128 == 0, "gemm_tile: row scale needs K % 128 == 0");
  const int epi = rsd ? TILE_EPI_RESID : rp ? TILE_EPI_ROPE : swiglu == 8 ? TILE_EPI_SWIGLU8 : swiglu ? TILE_EPI_SWIGLU : TILE_EPI_BF16;
  const int rs_np = rs ? K / 128 : 0;
  const TilePlan p = tile_plan(fmt, M, N, K, epi, (int)algo, tile_count_arg(grouped, E), tile_count_arg(rs, rs_np));
  // what tile_plan refused, by its code (the limits themselves: the table above tile_plan)
  static const char* const why[] = {
      "", "N % 16 == 0 (swiglu: % 256; rope, residual: % 128), K % 64 == 0, K >= 64, schedule (algo) 0 or 1, 1..256 "
      "experts; rope, the residual epilogue and the row scale are dense; the row scale goes with swiglu or rope and "
      "4..64 partial sums, a multiple of 4; it and the residual epilogue need schedule 1 and K >= 192",
      "more than 2^30 tiles", "w (one expert's), 256 rows of x and of resid must stay below 2^31 bytes (32-bit offsets)",
      "a quantised w is compiled for dense (not grouped) launches on schedule 1 (algo=1), swiglu 0 or 8 (no per-128 "
      "pairing), fp8 K >= 192, mxfp4 K >= 256 and K % 128 == 0"};
  TORCH_CHECK(p.err == 0, what, ": no form for N=", N, " K=", K, " (rc=", p.err, "): ", why[-p.err]);
  const void* sp = nullptr;
  if (fmt == TILE_W_F8) {
    TORCH_CHECK(wscale.has_value() && wscale->is_cuda() && wscale->scalar_type() == torch::kFloat32 &&
                    wscale->is_contiguous() && wscale->numel() == N,
                what, ": w needs its [N] fp32 scale vector");
    sp = wscale->data_ptr();
  } else if (fmt == TILE_W_F4) {
    TORCH_CHECK(wscale.has_value() && wscale->is_cuda() && wscale->scalar_type() == torch::kUInt8 &&
                    wscale->is_contiguous() && wscale->dim() == 4 && wscale->size(0) == w.size(0) &&
                    wscale->size(1) == w.size(1) && wscale->size(2) == 16 && wscale->size(3) == 4,
                what, ": w needs its [N/16, K/128, 16, 4] uint8 block scales");
    sp = wscale->data_ptr();
  } else {
    TORCH_CHECK(!wscale.has_value(), "gemm_tile: wscale goes with an fp8 or mxfp4 w");
  }
  TORCH_CHECK(y.dim() == 2 && y.size(0) == M && y.size(1) == (swiglu ? N / 2 : N), "gemm_tile: y shape");
  const int* op = nullptr;
  if (grouped) {
    dev_i32(*offsets, "offsets");
    TORCH_CHECK(offsets->numel() == E + 1, "gemm_tile: offsets must hold E + 1 entries");
    op = offsets->data_ptr<int>();
  }
  if (rp) {
    TORCH_CHECK(rope_cs.has_value(), "gemm_tile: rope_pos goes with rope_cs");
    dev_i32(*rope_pos, "rope_pos");
    TORCH_CHECK(rope_pos->numel() >= M, "gemm_tile: rope_pos needs a position per row");
    TORCH_CHECK(rope_heads >= 0 && rope_heads * 128 <= N, "gemm_tile: rope_heads * 128 must fit in N");
    TORCH_CHECK(rope_cs->is_cuda() && rope_cs->scalar_type() == torch::kFloat32 && rope_cs->is_contiguous() &&
                    rope_cs->dim() == 2 && rope_cs->size(1) == 128,
                "gemm_tile: rope_cs must be [max_pos, 128] fp32 (head_dim 128)");
  }
  // row scale (deferred RMSNorm of the A rows): rs_part [M][K / 128] fp32 partial sums of squares
  if (rs)
    TORCH_CHECK(rs_part->is_cuda() && rs_part->scalar_type() == torch::kFloat32 && rs_part->is_contiguous() &&
                    rs_part->dim() == 2 && rs_part->size(0) >= M && rs_part->size(1) == rs_np,
                "gemm_tile: rs_part must be [M, K / 128] fp32");
  // residual epilogue: resid [M][N] += y (in place), hw = resid * norm_w, ss_out [M][N / 128]
  if (rsd) {
    TORCH_CHECK(hw.has_value() && norm_w.has_value() && ss_out.has_value(),
                "gemm_tile: the residual epilogue goes with hw / norm_w / ss_out");
    dev_bf16(*resid, "resid"); dev_bf16(*hw, "hw"); dev_bf16(*norm_w, "norm_w");
    TORCH_CHECK(resid->is_contiguous() && resid->dim() == 2 && resid->size(0) == M && resid->size(1) == N,
                "gemm_tile: resid [M, N]");
    TORCH_CHECK(hw->is_contiguous() && hw->dim() == 2 && hw->size(0) == M && hw->size(1) == N, "gemm_tile: hw [M, N]");
    TORCH_CHECK(norm_w->is_contiguous() && norm_w->numel() == N, "gemm_tile: norm_w [N]");
    TORCH_CHECK(ss_out->is_cuda() && ss_out->scalar_type() == torch::kFloat32 && ss_out->is_contiguous() &&
                    ss_out->numel() >= (long)M * (N / 128), "gemm_tile: ss_out [M, N / 128] fp32");
  }
  check(k8sllm_gemm_tile(x.data_ptr(), w.data_ptr(), rsd ? resid->data_ptr() : y.data_ptr(), M, N, K, op, E,
                         (long)N * K, epi, (int)algo, rp ? rope_pos->data_ptr<int>() : nullptr,
                         rp ? rope_cs->data_ptr<float>() : nullptr, (int)rope_heads,
                         rs ? rs_part->data_ptr<float>() : nullptr, rs_np, (float)rs_eps,
                         rsd ? resid->data_ptr() : nullptr, rsd ? hw->data_ptr() : nullptr,
                         rsd ? norm_w->data_ptr() : nullptr, rsd ? ss_out->data_ptr<float>() : nullptr, wpk ? 1 : 0, sp,
                         fmt, (int)persist, (int)cus, cur()),
        what);
}

// tile_plan (gemm_tile_forms.h), what a launch with these arguments does: (err, schedule, row of
// gemm_tile_forms(), m-tiles, n-tiles, workgroups).  experts 0: a dense launch; rs_np 0: no row
// scale.  ext: two more - (.., the row of gemm_tile_persist_forms() that runs or -1 for the one-tile
// form, the grid) - for a device of `cus` CUs and the A/B override `persist` (-1: as the table routes).
// No launch.
std::vector<int64_t> gemm_tile_plan(int64_t fmt, int64_t M, int64_t N, int64_t K, int64_t epi, int64_t sch, int64_t experts,
                                    int64_t rs_np, int64_t persist, int64_t cus, bool ext) {
  const k8sllm::TilePlan p = k8sllm::tile_plan((int)fmt, (int)M, (int)N, (int)K, (int)epi, (int)sch, (int)experts,
                                               (int)rs_np, (int)persist, (int)cus);
  if (ext) return {p.err, p.sch, p.form, p.n_mt, p.n_nt, p.nwg, p.persist, p.grid};
  return {p.err, p.sch, p.form, p.n_mt, p.n_nt, p.nwg};
}

// The persistent instantiations of gemm_tile (kTilePersist): (epi, row scale, routed there by default) per row.
std::vector<std::vector<int64_t>> gemm_tile_persist_forms() {
  std::vector<int> v(3 * k8sllm::kTileNPersist);
  const int n = k8sllm_gemm_tile_persist_forms(v.data(), k8sllm::kTileNPersist);
  TORCH_CHECK(n == k8sllm::kTileNPersist, "gemm_tile_persist_forms: ", n, " rows compiled, ", k8sllm::kTileNPersist,
              " in the header");
  std::vector<std::vector<int64_t>> rows;
  for (int i = 0; i < n; ++i) rows.emplace_back(v.begin() + 3 * i, v.begin() + 3 * i + 3);
  return rows;
}

// The compiled forms of gemm_tile (kTileForms): (weight format, epi, grouped, row scale, also at
// schedule 0) per row.
std::vector<std::vector<int64_t>> gemm_tile_forms() {
  std::vector<int> v(5 * k8sllm::kTileNForms);
  const int n = k8sllm_gemm_tile_forms(v.data(), k8sllm::kTileNForms);
  TORCH_CHECK(n == k8sllm::kTileNForms, "gemm_tile_forms: ", n, " rows compiled, ", k8sllm::kTileNForms, " in the header");
  std::vector<std::vector<int64_t>> rows;
  for (int i = 0; i < n; ++i) rows.emplace_back(v.begin() + 5 * i, v.begin() + 5 * i + 5);
  return rows;
}

void gather_rows(torch::Tensor out, torch::Tensor x, torch::Tensor idx, int64_t div) {
  dev_bf16(out, "out"); dev_bf16(x, "x"); dev_i32(idx, "idx");
  TORCH_CHECK(out.is_contiguous() && x.is_contiguous(), "gather_rows contiguous");
  check(k8sllm_gather_rows(out.data_ptr(), x.data_ptr(), idx.data_ptr<int>(), idx.numel(), (int)x.size(1), (int)div,
                           cur()),
        "gather_rows");
}

}  // namespace

// Deferred RMSNorm operand: per-row partial sums of squares [M, nc] over nc equal column chunks
// of the K columns (add_norm_partial: 512-column chunks; the RESNORM epilogue: one per workgroup).
static void rownorm_args(const c10::optional<torch::Tensor>& rn_ss, int M, int K, const float*& rp, int& rn_nc) {
  if (!rn_ss.has_value()) return;
  TORCH_CHECK(rn_ss->is_cuda() && rn_ss->scalar_type() == torch::kFloat32 && rn_ss->is_contiguous() &&
                  rn_ss->dim() == 2 && rn_ss->size(0) >= M && rn_ss->size(1) >= 1 && K % rn_ss->size(1) == 0,
              "gemm_skinny: rn_ss must be [M, nc] fp32 with nc | K");
  rp = rn_ss->data_ptr<float>();
  rn_nc = (int)rn_ss->size(1);
}

// The fp32 slab buffer (split-K partials) of a decode GEMM: at least n elements.
static float* slab_buffer(const c10::optional<torch::Tensor>& partial, int64_t n, const char* what) {
  TORCH_CHECK(partial.has_value() && partial->is_cuda() && partial->scalar_type() == torch::kFloat32 &&
                  partial->is_contiguous() && partial->numel() >= n,
              what, ": partial must be a contiguous fp32 GPU tensor of at least ", n, " elements");
  return partial->data_ptr<float>();
}

// The packed SwiGLU output of a decode GEMM over N gate / up rows: [ceil(M/16), N/64, 64, 8] bf16,
// or with experts > 0 one per expert, [E, ceil(M/16), N/64, 64, 8].
static void* swiglu_packed_out(const c10::optional<torch::Tensor>& y, int experts, int M, int N, const char* what) {
  TORCH_CHECK(y.has_value(), what, ": output tensor required");
  dev_bf16(*y, "y");
  const int g = experts > 0 ? 1 : 0;
  TORCH_CHECK(y->dim() == 4 + g && y->is_contiguous() && (!g || y->size(0) == experts) &&
                  y->size(g) == (M + 15) / 16 && y->size(g + 1) * 64 == N && y->size(g + 2) == 64 &&
                  y->size(g + 3) == 8,
              what, ": packed SwiGLU output must be ", g ? "[E, " : "[", "ceil(M/16), N/64, 64, 8]");
  return y->data_ptr();
}

// Weight of a skinny GEMM: fragment-packed [N/16, K/32, 64, 8] (the model's one resident copy, or
// a copy kept for decode next to the row-major tensor), or the row-major [N, K] tensor itself
// (gemm_skinny_rm_kernel reads what prefill's GEMMs read).  `lead` = leading (expert) dimensions.
// Returns w_rm.
static int skinny_weight_dims(const torch::Tensor& wp, int lead, int& N, int& K, const char* what) {
  TORCH_CHECK(wp.is_contiguous(), what, ": weight must be contiguous");
  if (wp.dim() == lead + 4 && wp.size(lead + 2) == 64 && wp.size(lead + 3) == 8) {
    N = (int)wp.size(lead) * 16;
    K = (int)wp.size(lead + 1) * 32;
    return 0;
  }
  TORCH_CHECK(wp.dim() == lead + 2, what, ": weight must be fragment-packed [N/16, K/32, 64, 8] or row-major [N, K]");
  N = (int)wp.size(lead);
  K = (int)wp.size(lead + 1);
  TORCH_CHECK(N % 64 == 0 && K % 64 == 0, what, ": row-major weight needs N % 64 == 0 and K % 64 == 0");
  return 1;
}

// Skinny decode GEMM over a fragment-packed weight wp [N/16][K/32][64][8] or the row-major [N][K]
// weight (gemm_skinny.hip).
// epi 0: fp32 split-K slabs partial[S'][M][N], returns S'; epi 1: y = bf16(a . W^T);
// epi 2: y[M, N/2] = silu(gate) * up over a [32 gate | 32 up]-interleaved weight; epi 3: the same
// written fragment-packed.  Returns the
// number of slabs written (1 for epi 1/2).
int64_t gemm_skinny(torch::Tensor a, torch::Tensor wp, c10::optional<torch::Tensor> partial,
                    c10::optional<torch::Tensor> y, int64_t splits, int64_t epi, int64_t nt_tiles, int64_t rows,
                    c10::optional<torch::Tensor> rn_ss, double rn_eps, int64_t waves) {
  dev_bf16(a, "a"); dev_bf16(wp, "wp");
  int N, K;
  const int w_rm = skinny_weight_dims(wp, 0, N, K, "gemm_skinny");
  const bool a_packed = a.dim() == 4;
  TORCH_CHECK(!w_rm || a_packed, "gemm_skinny: a row-major weight needs a fragment-packed a");
  int M;
  if (a_packed) {  // fragment-packed activations [ceil(M/16), K/32, 64, 8]; `rows` = valid rows
    TORCH_CHECK(a.is_contiguous() && a.size(1) * 32 == K && a.size(2) == 64 && a.size(3) == 8,
                "gemm_skinny: packed a must be [ceil(M/16), K/32, 64, 8]");
    M = (int)rows;
    TORCH_CHECK(M > 0 && (M + 15) / 16 <= a.size(0), "gemm_skinny: rows exceed the packed a");
  } else {
    TORCH_CHECK(a.dim() == 2 && a.stride(1) == 1 && a.stride(0) % 8 == 0, "gemm_skinny: a layout");
    TORCH_CHECK(a.size(1) == K, "gemm_skinny: a has ", a.size(1), " columns, weight K=", K);
    M = (int)a.size(0);
  }
  const int S = epi == 0 ? (int)splits : 1;
  const auto p = k8sllm::skinny_plan(M, N, K, S, (int)epi, (int)nt_tiles, a_packed ? 1 : 0, (int)waves, 1, w_rm);
  TORCH_CHECK(p.err == 0, "gemm_skinny: at most ", k8sllm::kSkinnyMaxM, " rows of a shape it tiles, rc=", p.err);
  float* pp = nullptr;
  void* yp = nullptr;
  long ldy = 0;
  if (epi == 0) {
    pp = slab_buffer(partial, (int64_t)p.slabs * M * N, "gemm_skinny");
  } else if (epi == 3) {  // SwiGLU written fragment-packed [ceil(M/16), F/32, 64, 8]
    yp = swiglu_packed_out(y, 0, M, N, "gemm_skinny");
  } else {
    TORCH_CHECK(y.has_value(), "gemm_skinny: output tensor required");
    dev_bf16(*y, "y");
    const int ncol = epi == 2 ? N / 2 : N;
    TORCH_CHECK(y->dim() == 2 && y->size(0) >= M && y->size(1) == ncol && y->stride(1) == 1, "gemm_skinny: y shape");
    ldy = y->stride(0);
    yp = y->data_ptr();
  }
  const float* rp = nullptr;
  int rn_nc = 0;
  rownorm_args(rn_ss, M, K, rp, rn_nc);
  check(k8sllm_gemm_skinny(a.data_ptr(), a_packed ? 0 : a.stride(0), wp.data_ptr(), pp, yp, ldy, M, N, K, S, (int)epi,
                           (int)nt_tiles, a_packed ? 1 : 0, rp, rn_nc, K, (float)rn_eps, (int)waves, 1, 0, 0, 0,
                           nullptr, 0, w_rm, cur()),
        "gemm_skinny");
  return p.slabs;
}

// Decode GEMM with A shared through LDS (gemm_decode.hip), every weight format, dense or grouped;
// the tensors say which.  w.dtype: bf16 - fragment-packed [N/16, K/32, 64, 8] (ops.pack_skinny);
// float8_e4m3fn - codes [N/16, K/64, 64, 16] (ops.pack_skinny_f8) with wscale [N] fp32, one
// power-of-two scale per packed weight row; uint8 - mxfp4 codes [N/16, K/128, 64, 16] with wscale
// the e8m0 block scales [N/16, K/128, 16, 4] uint8 (ops.pack_skinny_f4).  For epi 2 the weight rows
// are interleaved per 16-row n-tile as [8 gate | 8 up].  One more leading dimension E on w (and
// wscale): a grouped launch over the local experts of a MoE layer (grid.z = expert).
// a packed [ceil(M/16), K/32, 64, 8] (`rows` valid); grouped: shared by every expert (gate_up) or
// [E, ceil(M/16), K/32, 64, 8] per expert (down).
// epi 0: fp32 slabs partial [S, M, N] ([E * S, M, N], scaled by row_w [M, E], the routing weights
// of these experts, where given); epi 1 (dense): y [M, N] bf16 (row stride y.stride(0)); epi 2:
// packed SwiGLU y [ceil(M/16), N/64, 64, 8] ([E, ...] per expert).  rn_ss: deferred RMSNorm of the
// A rows (dense).  f4_depth: the mxfp4 ring depth (8 / 16 k-steps), 0 = the launcher's choice.
// sw_rows / sw_wt / sw_xcd: ops.DEC_SLAB_ROWS / DEC_SLAB_WT / DEC_XCD_SPLITS (-1 as shipped, 0 off,
// 1 on; the shorter overload below passes -1): the slab epilogue's row-wide stores, their
// write-through form and the one-split-per-XCD placement - the slabs are the same bits either way.
// Row limit, slicing and forms are dec_plan's (gemm_dec_forms.h).  Returns the slab count (1 for
// epi 1 / 2); -1 if the configuration is not available (the caller falls back to gemm_skinny).
// delta / delta_slot / delta_slots (the longest overload; epi 2, dense, at most 16 deferred-norm
// sums per row): fp32 [M, N] over the packed row index, 16-byte aligned, added to the accumulator
// of the rows whose delta_slot[row] (int32 [M]) lies in [0, delta_slots) before gate and up are
// rounded; the other rows compute what a launch without delta computes.
int64_t gemm_dec_delta(torch::Tensor a, torch::Tensor w, c10::optional<torch::Tensor> wscale,
                       c10::optional<torch::Tensor> partial, c10::optional<torch::Tensor> y, int64_t splits, int64_t epi,
                       int64_t ntw, int64_t waves, int64_t depth, int64_t rows, c10::optional<torch::Tensor> rn_ss,
                       double rn_eps, c10::optional<torch::Tensor> row_w, int64_t f4_depth, int64_t sw_rows,
                       int64_t sw_wt, int64_t sw_xcd, c10::optional<torch::Tensor> delta,
                       c10::optional<torch::Tensor> delta_slot, int64_t delta_slots) {
  dev_bf16(a, "a");
  const auto wt = w.scalar_type();
  const int wf = wt == torch::kFloat8_e4m3fn ? k8sllm::DEC_W_F8 : wt == torch::kUInt8 ? k8sllm::DEC_W_F4 : k8sllm::DEC_W_BF16;
  const int g = w.dim() == 5 ? 1 : 0;  // grouped: leading expert dimension
  const int kq = wf == k8sllm::DEC_W_F4 ? 128 : wf == k8sllm::DEC_W_F8 ? 64 : 32, wl = wf == k8sllm::DEC_W_BF16 ? 8 : 16;
  const std::string whats = std::string("gemm_dec (") + (wf == k8sllm::DEC_W_F4 ? "mxfp4" : wf == k8sllm::DEC_W_F8 ? "fp8" : "bf16") +
                            (g ? ", grouped)" : ")");
  const char* what = whats.c_str();
  TORCH_CHECK(w.is_cuda() && (wf != k8sllm::DEC_W_BF16 || wt == torch::kBFloat16) && w.dim() == 4 + g &&
                  w.is_contiguous() && w.size(g + 2) == 64 && w.size(g + 3) == wl,
              what, ": w must be bf16 [N/16, K/32, 64, 8], float8_e4m3fn [N/16, K/64, 64, 16] or uint8 [N/16, K/128, "
                    "64, 16], fragment-packed, or an [E, ...] stack of such");
  const int E = g ? (int)w.size(0) : 0, N = (int)w.size(g) * 16, K = (int)w.size(g + 1) * kq, M = (int)rows;
  const void* sp = nullptr;
  if (wf == k8sllm::DEC_W_F8) {
    TORCH_CHECK(wscale.has_value() && wscale->is_cuda() && wscale->scalar_type() == torch::kFloat32 &&
                    wscale->is_contiguous() && (g ? wscale->dim() == 2 && wscale->size(0) == E && wscale->size(1) == N
                                                  : wscale->numel() == N),
                what, ": wscale must be [N] fp32 ([E, N] for a stack)");
    sp = wscale->data_ptr();
  } else if (wf == k8sllm::DEC_W_F4) {
    TORCH_CHECK(wscale.has_value() && wscale->is_cuda() && wscale->scalar_type() == torch::kUInt8 &&
                    wscale->is_contiguous() && wscale->dim() == 4 + g && (!g || wscale->size(0) == E) &&
                    wscale->size(g) == w.size(g) && wscale->size(g + 1) == w.size(g + 1) &&
                    wscale->size(g + 2) == 16 && wscale->size(g + 3) == 4,
                what, ": wscale must be uint8 [N/16, K/128, 16, 4] ([E, ...] for a stack)");
    sp = wscale->data_ptr();
  }
  TORCH_CHECK(g || !row_w.has_value(), what, ": routing weights go with an [E, ...] stack");
  TORCH_CHECK(!g || !rn_ss.has_value(), what, ": a grouped launch takes no deferred norm");
  TORCH_CHECK(!g || epi == 0 || epi == 2, what, ": only the slab and SwiGLU outputs");
  const float* rp = nullptr;
  int rn_nc = 0;
  rownorm_args(rn_ss, M, K, rp, rn_nc);
  const bool scaled = epi == 0 && row_w.has_value();  // (other epilogues have always ignored row_w)
  const k8sllm::DecPlan p = k8sllm::dec_plan(wf, M, N, K, (int)splits, (int)epi, (int)ntw, (int)waves, (int)depth,
                                             (int)f4_depth, E, scaled, rn_nc, (int)sw_rows, (int)sw_wt, (int)sw_xcd);
  const int MT = (M + 15) / 16;
  TORCH_CHECK(M > 0 && M <= p.max_m && (!g || E >= 1), what, ": 1..", p.max_m, " rows", g ? ", >= 1 expert" : "");
  const bool per_e = g && a.dim() == 5;
  const int ag = per_e ? 1 : 0;
  TORCH_CHECK(a.is_contiguous() && a.dim() == 4 + ag && (!per_e || a.size(0) == E) && a.size(ag) >= MT &&
                  a.size(ag + 1) * 32 == K && a.size(ag + 2) == 64 && a.size(ag + 3) == 8,
              what, ": a must be fragment-packed [ceil(M/16), K/32, 64, 8]", g ? " or [E, ...]" : "");
  const float* dp = nullptr;
  const int* dsp = nullptr;
  if (delta.has_value()) {
    TORCH_CHECK(epi == 2, what, ": a pre-activation delta goes with the SwiGLU epilogue (epi 2) only");
    TORCH_CHECK(!g && !row_w.has_value(), what, ": a grouped launch takes no delta");
    TORCH_CHECK(rn_nc <= k8sllm::kDecRnNarrow, what, ": a delta goes with at most ", k8sllm::kDecRnNarrow,
                " deferred-norm sums per row, not ", rn_nc);
    TORCH_CHECK(delta->is_cuda() && delta->scalar_type() == torch::kFloat32 && delta->is_contiguous() &&
                    delta->numel() >= (int64_t)M * N && reinterpret_cast<uintptr_t>(delta->data_ptr()) % 16 == 0 &&
                    (int64_t)M * N * 4 < 0x7fffffffLL,
                what, ": delta must be fp32, contiguous, 16-byte aligned, [M, N] under 2 GiB");
    TORCH_CHECK(delta_slot.has_value() && delta_slot->is_cuda() && delta_slot->scalar_type() == torch::kInt32 &&
                    delta_slot->is_contiguous() && delta_slot->numel() >= M && delta_slots >= 1,
                what, ": delta_slot must be int32 [M] with delta_slots >= 1");
    dp = delta->data_ptr<float>();
    dsp = delta_slot->data_ptr<int>();
  }
  if (p.err < 0) return -1;
  float* pp = nullptr;
  void* yp = nullptr;
  long ldy = 0, y_es = 0;
  const float* rw = nullptr;
  int rw_ld = 0;
  if (epi == 0) {
    pp = slab_buffer(partial, (int64_t)p.slabs * M * N, what);
    if (scaled) {
      TORCH_CHECK(row_w->is_cuda() && row_w->scalar_type() == torch::kFloat32 && row_w->dim() == 2 &&
                      row_w->size(0) >= M && row_w->size(1) == E && row_w->stride(1) == 1,
                  what, ": row_w [M, E] fp32");
      rw = row_w->data_ptr<float>();
      rw_ld = (int)row_w->stride(0);
    }
  } else if (epi == 2) {
    yp = swiglu_packed_out(y, E, M, N, what);
    y_es = g ? y->stride(0) : 0;
  } else {
    TORCH_CHECK(y.has_value(), what, ": output tensor required");
    dev_bf16(*y, "y");
    TORCH_CHECK(y->dim() == 2 && y->size(0) >= M && y->size(1) == N && y->stride(1) == 1, what, ": y [M, N]");
    ldy = y->stride(0);
    yp = y->data_ptr();
  }
  // the kernel strides W and the scales in bytes
  const long a_es = per_e ? a.stride(0) : 0, w_eb = g ? w.stride(0) * w.element_size() : 0;
  const long s_eb = g && sp ? wscale->stride(0) * wscale->element_size() : 0;
  const int rc = k8sllm_gemm_dec(a.data_ptr(), w.data_ptr(), sp, wf, pp, yp, ldy, M, N, K, (int)splits, (int)epi,
                                 (int)ntw, (int)waves, (int)depth, (int)f4_depth, rp, rn_nc, K, (float)rn_eps, E,
                                 a_es, w_eb, s_eb, y_es, rw, rw_ld, (int)sw_rows, (int)sw_wt, (int)sw_xcd, dp, dsp,
                                 (int)delta_slots, cur());
  if (rc < 0) return -1;
  check(rc, what);
  return p.slabs;
}

int64_t gemm_dec_sw(torch::Tensor a, torch::Tensor w, c10::optional<torch::Tensor> wscale,
                    c10::optional<torch::Tensor> partial, c10::optional<torch::Tensor> y, int64_t splits, int64_t epi,
                    int64_t ntw, int64_t waves, int64_t depth, int64_t rows, c10::optional<torch::Tensor> rn_ss,
                    double rn_eps, c10::optional<torch::Tensor> row_w, int64_t f4_depth, int64_t sw_rows,
                    int64_t sw_wt, int64_t sw_xcd) {
  return gemm_dec_delta(a, w, wscale, partial, y, splits, epi, ntw, waves, depth, rows, rn_ss, rn_eps, row_w, f4_depth,
                        sw_rows, sw_wt, sw_xcd, c10::nullopt, c10::nullopt, 0);
}

int64_t gemm_dec(torch::Tensor a, torch::Tensor w, c10::optional<torch::Tensor> wscale,
                 c10::optional<torch::Tensor> partial, c10::optional<torch::Tensor> y, int64_t splits, int64_t epi,
                 int64_t ntw, int64_t waves, int64_t depth, int64_t rows, c10::optional<torch::Tensor> rn_ss,
                 double rn_eps, c10::optional<torch::Tensor> row_w, int64_t f4_depth) {
  return gemm_dec_sw(a, w, wscale, partial, y, splits, epi, ntw, waves, depth, rows, rn_ss, rn_eps, row_w, f4_depth,
                     -1, -1, -1);
}

// dec_plan (gemm_dec_forms.h), what a launch with these arguments does: (err, m-tiles, kchunk,
// mxfp4 ring depth, wide-norm, grid x, y, z, slabs, row limit, row-wide slab stores, write-through, one
// split per XCD).  experts 0: a dense launch.  sw_*: the three switches (the shorter overload: -1, as
// shipped).  No launch.
std::vector<int64_t> gemm_dec_plan_sw(int64_t wf, int64_t M, int64_t N, int64_t K, int64_t splits, int64_t epi,
                                      int64_t ntw, int64_t waves, int64_t depth, int64_t f4_depth, int64_t experts,
                                      bool has_row_w, int64_t rn_nc, int64_t sw_rows, int64_t sw_wt, int64_t sw_xcd) {
  const k8sllm::DecPlan p = k8sllm::dec_plan((int)wf, (int)M, (int)N, (int)K, (int)splits, (int)epi, (int)ntw,
                                             (int)waves, (int)depth, (int)f4_depth, (int)experts, has_row_w, (int)rn_nc,
                                             (int)sw_rows, (int)sw_wt, (int)sw_xcd);
  return {p.err, p.mt, p.kchunk, p.d4, p.rnw, p.gx, p.gy, p.gz, p.slabs, p.max_m, p.rows, p.wt, p.xcd};
}

std::vector<int64_t> gemm_dec_plan(int64_t wf, int64_t M, int64_t N, int64_t K, int64_t splits, int64_t epi, int64_t ntw,
                                   int64_t waves, int64_t depth, int64_t f4_depth, int64_t experts, bool has_row_w,
                                   int64_t rn_nc) {
  return gemm_dec_plan_sw(wf, M, N, K, splits, epi, ntw, waves, depth, f4_depth, experts, has_row_w, rn_nc, -1, -1, -1);
}

// The rows of kDecForms with fp8-weight instantiations (kDecF8Forms), as indices into gemm_dec_forms().
std::vector<int64_t> gemm_dec_f8_forms() {
  std::vector<int> v(k8sllm::kDecNF8Forms);
  const int n = k8sllm_gemm_dec_f8_forms(v.data(), k8sllm::kDecNF8Forms);
  TORCH_CHECK(n == k8sllm::kDecNF8Forms, "gemm_dec_f8_forms: ", n, " rows compiled, ", k8sllm::kDecNF8Forms,
              " in the header");
  return std::vector<int64_t>(v.begin(), v.end());
}

// The rows of kDecForms with mxfp4-weight instantiations (kDecF4Forms): (index into
// gemm_dec_forms(), F4 ring depth at one m-tile) each.
std::vector<std::vector<int64_t>> gemm_dec_f4_forms() {
  std::vector<int> v(2 * k8sllm::kDecNF4Forms);
  const int n = k8sllm_gemm_dec_f4_forms(v.data(), k8sllm::kDecNF4Forms);
  TORCH_CHECK(n == k8sllm::kDecNF4Forms, "gemm_dec_f4_forms: ", n, " rows compiled, ", k8sllm::kDecNF4Forms,
              " in the header");
  std::vector<std::vector<int64_t>> out;
  for (int i = 0; i < n; ++i) out.push_back({v[2 * i], v[2 * i + 1]});
  return out;
}

// The compiled forms of gemm_dec (kDecForms): (epi, ntw, waves, depth, max m-tiles, wide-norm) per row.
std::vector<std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>> gemm_dec_forms() {
  std::vector<int> v(6 * k8sllm::kDecNForms);
  const int n = k8sllm_gemm_dec_forms(v.data(), k8sllm::kDecNForms);
  TORCH_CHECK(n == k8sllm::kDecNForms, "gemm_dec_forms: ", n, " rows compiled, ", k8sllm::kDecNForms,
              " in the header");
  std::vector<std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>> rows;
  for (int i = 0; i < n; ++i)
    rows.emplace_back(v[6 * i], v[6 * i + 1], v[6 * i + 2], v[6 * i + 3], v[6 * i + 4], v[6 * i + 5]);
  return rows;
}

// The compiled forms of gemm_skinny (kSkinnyForms): (family, epi, nt, waves, a_packed, min m-tiles,
// max m-tiles) per row.
std::vector<std::vector<int64_t>> gemm_skinny_forms() {
  std::vector<std::vector<int64_t>> rows;
  for (const k8sllm::SkinnyForm& f : k8sllm::kSkinnyForms)
    rows.push_back({f.family, f.epi, f.nt, f.waves, f.a_packed, f.min_mt, f.max_mt});
  return rows;
}

// skinny_plan (gemm_skinny_plan.h), what a launch with these arguments does: (err, family, m-tiles,
// nt, waves, kchunk, slabs, grid x).  No launch.
std::vector<int64_t> gemm_skinny_plan(int64_t M, int64_t N, int64_t K, int64_t S, int64_t epi, int64_t nt_tiles,
                                      int64_t a_packed, int64_t waves, int64_t experts, int64_t w_rm) {
  const k8sllm::SkinnyPlan p = k8sllm::skinny_plan((int)M, (int)N, (int)K, (int)S, (int)epi, (int)nt_tiles,
                                                   (int)a_packed, (int)waves, (int)experts, (int)w_rm);
  return {p.err, p.family, p.mt, p.nt, p.waves, p.kchunk, p.slabs, p.gx};
}

// Row-complete decode GEMM + residual add + deferred-norm operands (gemm_decode.hip
// gemm_dec_rc_kernel): a packed [ceil(M/16), K/32, 64, 8] (`rows` valid), wp packed [N/16, K/32,
// 64, 8]; resid [M, N] bf16 += a . wp^T (in place); xw packed [ceil(M/16), N/32, 64, 8] = resid *
// nw; ss [M, N/16] fp32 per-16-column sums of resid^2.  Returns false for a shape it does not tile.
bool gemm_dec_rc(torch::Tensor a, torch::Tensor wp, torch::Tensor resid, torch::Tensor nw, torch::Tensor xw,
                 torch::Tensor ss, int64_t rows) {
  dev_bf16(a, "a"); dev_bf16(wp, "wp"); dev_bf16(resid, "resid"); dev_bf16(nw, "nw"); dev_bf16(xw, "xw");
  TORCH_CHECK(wp.dim() == 4 && wp.is_contiguous() && wp.size(2) == 64 && wp.size(3) == 8, "gemm_dec_rc: wp packed");
  const int N = (int)wp.size(0) * 16, K = (int)wp.size(1) * 32, M = (int)rows;
  TORCH_CHECK(a.dim() == 4 && a.is_contiguous() && a.size(1) * 32 == K && a.size(2) == 64 && a.size(3) == 8 &&
                  M > 0 && M <= k8sllm::kDecNarrowMaxM && (M + 15) / 16 <= a.size(0), "gemm_dec_rc: a packed [ceil(M/16), K/32, 64, 8]");
  TORCH_CHECK(resid.dim() == 2 && resid.is_contiguous() && resid.size(0) >= M && resid.size(1) == N,
              "gemm_dec_rc: resid [M, N]");
  TORCH_CHECK(nw.numel() == N && nw.is_contiguous(), "gemm_dec_rc: nw [N]");
  TORCH_CHECK(xw.dim() == 4 && xw.is_contiguous() && xw.size(0) == (M + 15) / 16 && xw.size(1) * 32 == N,
              "gemm_dec_rc: xw packed [ceil(M/16), N/32, 64, 8]");
  TORCH_CHECK(ss.is_cuda() && ss.scalar_type() == torch::kFloat32 && ss.is_contiguous() && ss.dim() == 2 &&
                  ss.size(0) >= M && ss.size(1) == N / 16, "gemm_dec_rc: ss [M, N/16] fp32");
  const int rc = k8sllm_gemm_dec_rc(a.data_ptr(), wp.data_ptr(), resid.data_ptr(), nw.data_ptr(), xw.data_ptr(),
                                    ss.data_ptr<float>(), M, N, K, cur());
  if (rc == -1) return false;
  check(rc, "gemm_dec_rc");
  return true;
}

// Grouped (MoE) skinny GEMM: wp [E, N/16, K/32, 64, 8] (one packed weight per local expert).
// a: packed [MT, K/32, 64, 8] shared by every expert, or [E, MT, K/32, 64, 8] per expert.
// epi 3: y = packed SwiGLU [E, MT, F/32, 64, 8]; epi 0: fp32 slabs partial[E * S'][M][N] with
// row m of expert x's output scaled by row_w[m][x] (row_w [M, E] fp32, routing weights).
// Returns E * S' (the slab count for the residual-add kernels) or 1.
int64_t gemm_skinny_grouped(torch::Tensor a, torch::Tensor wp, c10::optional<torch::Tensor> partial,
                            c10::optional<torch::Tensor> y, int64_t splits, int64_t epi, int64_t rows,
                            c10::optional<torch::Tensor> row_w, int64_t waves) {
  dev_bf16(a, "a"); dev_bf16(wp, "wp");
  int N, K;
  const int w_rm = skinny_weight_dims(wp, 1, N, K, "gemm_skinny_grouped");
  TORCH_CHECK(epi == 0 || epi == 3, "gemm_skinny_grouped: epi must be 0 (slabs) or 3 (packed SwiGLU)");
  const int E = (int)wp.size(0), M = (int)rows;
  const long w_es = wp[0].numel();
  const int S = epi == 0 && splits > 0 ? (int)splits : 1;
  const auto p = k8sllm::skinny_plan(M, N, K, S, (int)epi, 4, 1, (int)waves, E, w_rm);
  TORCH_CHECK(M > 0 && p.err == 0, "gemm_skinny_grouped: 1..", k8sllm::kSkinnyMaxM, " rows (1..",
              k8sllm::kSkinnyGroupedMaxM, " over row-major weights of 2+ experts) of a shape it tiles, rc=", p.err);
  const int MT = p.mt;
  long a_es = 0;
  TORCH_CHECK(a.is_contiguous() && a.size(-1) == 8 && a.size(-2) == 64 && a.size(-3) * 32 == K,
              "gemm_skinny_grouped: a must be fragment-packed with K = ", K);
  if (a.dim() == 5) {
    TORCH_CHECK(a.size(0) == E && a.size(1) == MT, "gemm_skinny_grouped: per-expert a must be [E, MT, K/32, 64, 8]");
    a_es = a[0].numel();
  } else {
    TORCH_CHECK(a.dim() == 4 && a.size(0) == MT, "gemm_skinny_grouped: shared a must be [MT, K/32, 64, 8]");
  }
  float* pp = nullptr;
  void* yp = nullptr;
  long y_es = 0;
  const float* rw = nullptr;
  if (epi == 0) {
    pp = slab_buffer(partial, (int64_t)E * p.slabs * M * N, "gemm_skinny_grouped");
    if (row_w.has_value()) {
      TORCH_CHECK(row_w->is_cuda() && row_w->scalar_type() == torch::kFloat32 && row_w->is_contiguous() &&
                      row_w->dim() == 2 && row_w->size(0) >= M && row_w->size(1) == E,
                  "gemm_skinny_grouped: row_w must be [M, E] fp32");
      rw = row_w->data_ptr<float>();
    }
  } else {
    yp = swiglu_packed_out(y, E, M, N, "gemm_skinny_grouped");
    y_es = y->stride(0);
  }
  check(k8sllm_gemm_skinny(a.data_ptr(), 0, wp.data_ptr(), pp, yp, 0, M, N, K, S, (int)epi, 4, 1, nullptr, 0, K, 0.f,
                           (int)waves, E, w_es, a_es, y_es, rw, E, w_rm, cur()),
        "gemm_skinny_grouped");
  return epi == 0 ? (int64_t)E * p.slabs : 1;
}

// residual += sum of S slabs; out = residual * w (row-major or fragment-packed); ss_part[m][c] =
// sum of residual^2 over columns [512 c, 512 c + 512) - the deferred-RMSNorm producer.
// decode front end: resolved ids -> embedding rows (residual) + the first layer's deferred-norm operands
void embed_norm_partial(torch::Tensor out, torch::Tensor residual, torch::Tensor ids, c10::optional<torch::Tensor> src,
                        c10::optional<torch::Tensor> prev, torch::Tensor emb, torch::Tensor w, torch::Tensor ss_part) {
  dev_bf16(out, "out"); dev_bf16(residual, "residual"); dev_bf16(emb, "emb"); dev_bf16(w, "w"); dev_i32(ids, "ids");
  TORCH_CHECK(residual.is_contiguous() && residual.dim() == 2 && emb.is_contiguous() && emb.dim() == 2 &&
                  w.is_contiguous(), "embed_norm_partial layout");
  const int M = (int)residual.size(0), d = (int)residual.size(1);
  TORCH_CHECK(d % 512 == 0 && emb.size(1) == d && w.numel() == d && ids.numel() >= M, "embed_norm_partial shapes");
  TORCH_CHECK(src.has_value() == prev.has_value(), "embed_norm_partial: src and prev go together");
  const int* sp = nullptr;
  const int* pp = nullptr;
  if (src.has_value()) {
    dev_i32(*src, "src"); dev_i32(*prev, "prev");
    TORCH_CHECK(src->numel() >= M, "embed_norm_partial: src [M]");
    sp = src->data_ptr<int>();
    pp = prev->data_ptr<int>();
  }
  TORCH_CHECK(ss_part.is_cuda() && ss_part.scalar_type() == torch::kFloat32 && ss_part.is_contiguous() &&
                  ss_part.numel() >= (int64_t)M * (d / 512), "ss_part");
  long ostride = d;
  if (out.dim() == 4) {
    TORCH_CHECK(out.size(0) == (M + 15) / 16 && out.size(1) * 32 == d && out.size(2) == 64 && out.size(3) == 8,
                "packed out must be [ceil(M/16), d/32, 64, 8]");
    ostride = -(long)(d / 32);
  } else {
    TORCH_CHECK(out.numel() == (int64_t)M * d, "out shape");
  }
  check(k8sllm_embed_norm_partial(out.data_ptr(), ostride, residual.data_ptr(), ids.data_ptr<int>(), sp, pp,
                                  emb.data_ptr(), (int)emb.size(0), w.data_ptr(), M, d, ss_part.data_ptr<float>(), cur()),
        "embed_norm_partial");
}

void add_norm_partial(torch::Tensor out, torch::Tensor residual, c10::optional<torch::Tensor> partial, int64_t S,
                      torch::Tensor w, torch::Tensor ss_part) {
  dev_bf16(out, "out"); dev_bf16(residual, "residual"); dev_bf16(w, "w");
  TORCH_CHECK(residual.is_contiguous() && out.is_contiguous() && w.is_contiguous() && residual.dim() == 2,
              "add_norm_partial layout");
  const int M = (int)residual.size(0), d = (int)residual.size(1);
  TORCH_CHECK(d % 512 == 0, "add_norm_partial: d % 512 != 0");
  TORCH_CHECK(ss_part.is_cuda() && ss_part.scalar_type() == torch::kFloat32 && ss_part.is_contiguous() &&
                  ss_part.numel() >= (int64_t)M * (d / 512), "ss_part");
  const float* pp = nullptr;
  if (S > 0) {
    TORCH_CHECK(partial.has_value() && partial->scalar_type() == torch::kFloat32 && partial->is_contiguous() &&
                    partial->numel() >= S * M * d, "partial");
    pp = partial->data_ptr<float>();
  }
  long ostride = d;
  if (out.dim() == 4) {
    TORCH_CHECK(out.size(0) == (M + 15) / 16 && out.size(1) * 32 == d && out.size(2) == 64 && out.size(3) == 8,
                "packed out must be [ceil(M/16), d/32, 64, 8]");
    ostride = -(long)(d / 32);
  } else {
    TORCH_CHECK(out.numel() == (int64_t)M * d, "out shape");
  }
  check(k8sllm_add_norm_partial(out.data_ptr(), ostride, residual.data_ptr(), pp, (int)S, M, w.data_ptr(), d,
                                ss_part.data_ptr<float>(), cur()),
        "add_norm_partial");
}

void reduce_slabs(torch::Tensor out, torch::Tensor partial, int64_t S) {
  dev_bf16(out, "out");
  TORCH_CHECK(out.is_contiguous(), "reduce_slabs: out must be contiguous");
  TORCH_CHECK(partial.is_cuda() && partial.scalar_type() == torch::kFloat32 && partial.is_contiguous(), "partial");
  TORCH_CHECK(partial.numel() >= S * out.numel(), "reduce_slabs: partial too small");
  check(k8sllm_reduce_slabs(out.data_ptr(), partial.data_ptr<float>(), (int)S, out.numel(), cur()), "reduce_slabs");
}

// Per-request LoRA (lora.hip, ops.lora_slab / ops.lora_add).  K slices of a shrink launch over depth K.
int64_t lora_shrink_plan(int64_t K) { return k8sllm_lora_shrink_plan((int)K); }

// t_part [S, M, R] fp32 = A[slot[row]] . x[row] per K slice; x fragment-packed [ceil(M/16), K/32, 64, 8] or
// row-major [M, K]; A [slots, R, K] bf16; slot int32 [>= M] (-1: no adapter); ss_part [>= M, cols] fp32: the
// deferred RMSNorm's partial sums of squares.  Returns S.
int64_t lora_shrink(torch::Tensor x, torch::Tensor A, torch::Tensor slot, torch::Tensor t_part, int64_t rows,
                    c10::optional<torch::Tensor> ss_part, double eps) {
  dev_bf16(x, "x"); dev_bf16(A, "A"); dev_i32(slot, "slot");
  TORCH_CHECK(A.dim() == 3 && A.is_contiguous(), "lora_shrink: A [slots, R, K]");
  const int nslots = (int)A.size(0), R = (int)A.size(1), K = (int)A.size(2);
  const long M = rows;
  const int S = k8sllm_lora_shrink_plan(K);
  TORCH_CHECK(S > 0 && R % 16 == 0 && M > 0 && nslots > 0, "lora_shrink: K % 32, R % 16, rows > 0");
  const bool packed = x.dim() == 4;
  long xstride = 0;
  if (packed) {
    TORCH_CHECK(x.is_contiguous() && x.size(0) == (M + 15) / 16 && x.size(1) * 32 == K && x.size(2) == 64 &&
                    x.size(3) == 8, "lora_shrink: packed x must be [ceil(M/16), K/32, 64, 8]");
  } else {
    TORCH_CHECK(x.dim() == 2 && x.size(0) >= M && x.size(1) == K && x.stride(1) == 1 && x.stride(0) % 8 == 0 &&
                    (uintptr_t)x.data_ptr() % 16 == 0, "lora_shrink: x [M, K] bf16 rows, 16-byte aligned");
    xstride = x.stride(0);
  }
  TORCH_CHECK(slot.is_contiguous() && slot.numel() >= M, "lora_shrink: slot int32 [M]");
  TORCH_CHECK(t_part.is_cuda() && t_part.scalar_type() == torch::kFloat32 && t_part.is_contiguous() &&
                  t_part.numel() >= (int64_t)S * M * R, "lora_shrink: t_part fp32 [S, M, R]");
  const float* ss = nullptr;
  int cols = 0;
  if (ss_part.has_value()) {
    TORCH_CHECK(ss_part->is_cuda() && ss_part->scalar_type() == torch::kFloat32 && ss_part->is_contiguous() &&
                    ss_part->dim() == 2 && ss_part->size(0) >= M, "lora_shrink: ss_part fp32 [M, cols]");
    ss = ss_part->data_ptr<float>();
    cols = (int)ss_part->size(1);
  }
  check(k8sllm_lora_shrink(x.data_ptr(), packed ? 1 : 0, xstride, A.data_ptr(), slot.data_ptr<int>(), ss, cols,
                           (float)eps, t_part.data_ptr<float>(), M, R, K, nslots, cur()),
        "lora_shrink");
  return S;
}

// delta = scaling[slot] * B[slot] . sum_s t_part[s]: into the fp32 slab ``slab_index`` of ``out`` ([.., M, N]
// slabs; rows without an adapter written as zeros), or added in place to bf16 ``out`` [M, N] (slab_index < 0).
void lora_expand(torch::Tensor t_part, int64_t S, torch::Tensor B, torch::Tensor scaling, torch::Tensor slot,
                 torch::Tensor out, int64_t rows, int64_t slab_index) {
  dev_bf16(B, "B"); dev_i32(slot, "slot");
  TORCH_CHECK(B.dim() == 3 && B.is_contiguous(), "lora_expand: B [slots, N, R]");
  const int nslots = (int)B.size(0), N = (int)B.size(1), R = (int)B.size(2);
  const long M = rows;
  TORCH_CHECK(S > 0 && M > 0 && N % 16 == 0 && R % 32 == 0 && R <= 224, "lora_expand: N % 16, R % 32, R <= 224");
  TORCH_CHECK(t_part.is_cuda() && t_part.scalar_type() == torch::kFloat32 && t_part.is_contiguous() &&
                  t_part.numel() >= S * M * R, "lora_expand: t_part fp32 [S, M, R]");
  TORCH_CHECK(scaling.is_cuda() && scaling.scalar_type() == torch::kFloat32 && scaling.is_contiguous() &&
                  scaling.numel() == nslots, "lora_expand: scaling fp32 [slots]");
  TORCH_CHECK(slot.is_contiguous() && slot.numel() >= M, "lora_expand: slot int32 [M]");
  float* slab = nullptr;
  void* y = nullptr;
  long ystride = 0;
  if (slab_index >= 0) {
    TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kFloat32 && out.is_contiguous() &&
                    out.numel() >= (slab_index + 1) * M * N, "lora_expand: workspace too small for the slab");
    slab = out.data_ptr<float>() + slab_index * M * N;
  } else {
    dev_bf16(out, "y");
    TORCH_CHECK(out.dim() == 2 && out.size(0) >= M && out.size(1) == N && out.stride(1) == 1,
                "lora_expand: y [M, N] bf16 rows");
    y = out.data_ptr();
    ystride = out.stride(0);
  }
  check(k8sllm_lora_expand(t_part.data_ptr<float>(), (int)S, B.data_ptr(), scaling.data_ptr<float>(),
                           slot.data_ptr<int>(), slab, y, ystride, M, N, R, nslots, cur()),
        "lora_expand");
}

void reduce_add_rms_norm(torch::Tensor out, torch::Tensor residual, c10::optional<torch::Tensor> partial, int64_t S,
                         torch::Tensor w, double eps, c10::optional<torch::Tensor> out_packed) {
  dev_bf16(out, "out"); dev_bf16(residual, "residual"); dev_bf16(w, "w");
  TORCH_CHECK(residual.is_contiguous() && out.is_contiguous() && w.is_contiguous(), "reduce_add_rms_norm layout");
  const int d = (int)residual.size(-1);
  const int M = (int)(residual.numel() / d);
  const float* pp = nullptr;
  if (S > 0) {
    TORCH_CHECK(partial.has_value() && partial->is_cuda() && partial->scalar_type() == torch::kFloat32 &&
                    partial->is_contiguous(), "partial");
    TORCH_CHECK(partial->numel() >= S * M * d, "reduce_add_rms_norm: partial too small");
    pp = partial->data_ptr<float>();
  }
  long ostride = d;
  if (out.dim() == 4) {  // fragment-packed [ceil(M/16), d/32, 64, 8] for the next gemm_skinny
    TORCH_CHECK(out.size(0) == (M + 15) / 16 && out.size(1) * 32 == d && out.size(2) == 64 && out.size(3) == 8,
                "packed out must be [ceil(M/16), d/32, 64, 8]");
    ostride = -(long)(d / 32);
  } else {
    TORCH_CHECK(out.numel() == (int64_t)M * d, "reduce_add_rms_norm shapes");
  }
  void* out2 = nullptr;
  if (out_packed.has_value()) {  // a second, fragment-packed copy of the normed rows
    const auto& o2 = *out_packed;
    dev_bf16(o2, "out_packed");
    TORCH_CHECK(o2.dim() == 4 && o2.is_contiguous() && o2.size(0) == (M + 15) / 16 && o2.size(1) * 32 == d &&
                    o2.size(2) == 64 && o2.size(3) == 8, "out_packed must be [ceil(M/16), d/32, 64, 8]");
    out2 = o2.data_ptr();
  }
  check(k8sllm_reduce_add_rmsnorm(out.data_ptr(), residual.data_ptr(), pp, (int)S, M, w.data_ptr(), d, (float)eps,
                                  ostride, out2, cur()),
        "reduce_add_rms_norm");
}

// One-shot IPC all-reduce (custom_ar.hip).  The state is an opaque pointer held by Python.
py::tuple car_create(int64_t rank, int64_t world, int64_t max_elems) {
  std::string h(2 * k8sllm_car_handle_size(), '\0');
  int err = 0;
  void* st = k8sllm_car_create((int)rank, (int)world, (long)max_elems, h.data(), &err);
  TORCH_CHECK(st != nullptr, "custom all-reduce: allocation / IPC handle failed, hip error ", err);
  return py::make_tuple((int64_t)(intptr_t)st, py::bytes(h));
}

void car_open(int64_t state, py::bytes all_handles) {
  std::string a = all_handles;
  check(k8sllm_car_open((void*)(intptr_t)state, a.data()), "car_open (hipIpcOpenMemHandle)");
}

void car_all_reduce(int64_t state, torch::Tensor in, torch::Tensor out, int64_t spin_limit, int64_t algo) {
  dev_bf16(in, "in"); dev_bf16(out, "out");
  TORCH_CHECK(in.is_contiguous() && out.is_contiguous() && in.numel() == out.numel(), "car_all_reduce layout");
  check(k8sllm_car_all_reduce((void*)(intptr_t)state, in.data_ptr(), out.data_ptr(), (long)in.numel(),
                              (long)spin_limit, (int)algo, cur()),
        "car_all_reduce");
}

// TP row-parallel tail in one launch: slabs [ns, M, d] fp32 -> reduced over ranks -> residual +=,
// RMSNorm * w -> out (row-major [M, d] or fragment-packed when packed).
void car_fused_tail(int64_t state, torch::Tensor slabs, int64_t ns, torch::Tensor residual, torch::Tensor w,
                    torch::Tensor out, double eps, bool packed, int64_t spin_limit, int64_t algo) {
  dev_bf16(residual, "residual"); dev_bf16(w, "w"); dev_bf16(out, "out");
  TORCH_CHECK(slabs.is_cuda() && slabs.scalar_type() == torch::kFloat32 && slabs.is_contiguous(), "slabs fp32");
  TORCH_CHECK(residual.dim() == 2 && residual.is_contiguous() && w.is_contiguous() && out.is_contiguous(),
              "car_fused_tail layout");
  const int M = (int)residual.size(0), d = (int)residual.size(1);
  TORCH_CHECK(slabs.numel() >= ns * (long)M * d && w.numel() == d, "car_fused_tail sizes");
  TORCH_CHECK(packed ? out.numel() >= (long)((M + 15) / 16) * 16 * d : out.numel() >= (long)M * d,
              "car_fused_tail out size");
  check(k8sllm_car_fused_tail((void*)(intptr_t)state, slabs.data_ptr<float>(), (int)ns, (long)M * d,
                              residual.data_ptr(), w.data_ptr(), out.data_ptr(), d, M, d, (float)eps, packed ? 1 : 0,
                              (long)spin_limit, (int)algo, cur()),
        "car_fused_tail");
}

void car_all_gather(int64_t state, torch::Tensor in, torch::Tensor out, int64_t spin_limit) {
  dev_bf16(in, "in"); dev_bf16(out, "out");
  TORCH_CHECK(in.is_contiguous() && out.is_contiguous() && out.numel() % in.numel() == 0 &&
                  out.data_ptr() != in.data_ptr(), "car_all_gather layout");
  check(k8sllm_car_all_gather((void*)(intptr_t)state, in.data_ptr(), out.data_ptr(), (long)in.numel(),
                              (long)spin_limit, cur()),
        "car_all_gather");
}

void car_all_to_all(int64_t state, torch::Tensor in, torch::Tensor out, int64_t spin_limit) {
  dev_bf16(in, "in"); dev_bf16(out, "out");
  TORCH_CHECK(in.is_contiguous() && out.is_contiguous() && out.numel() == in.numel() &&
                  out.data_ptr() != in.data_ptr(), "car_all_to_all layout");
  check(k8sllm_car_all_to_all((void*)(intptr_t)state, in.data_ptr(), out.data_ptr(), (long)in.numel(),
                              (long)spin_limit, cur()),
        "car_all_to_all");
}

int64_t car_error(int64_t state) { return k8sllm_car_error((void*)(intptr_t)state); }

void car_error_async(int64_t state, torch::Tensor host) {
  TORCH_CHECK(!host.is_cuda() && host.scalar_type() == torch::kInt32 && host.numel() >= 1, "host int32 flag");
  check(k8sllm_car_error_async((void*)(intptr_t)state, host.data_ptr(), cur()), "car_error_async");
}

void car_destroy(int64_t state) { k8sllm_car_destroy((void*)(intptr_t)state); }

PYBIND11_MODULE(_k8sllm_ops, m) {
  m.doc() = "gfx950 HIP kernels for k8s-llm-monitor-amd";
  m.def("rms_norm", &rms_norm);
  m.def("fused_add_rms_norm", &fused_add_rms_norm);
  m.def("layer_norm", &layer_norm);
  m.def("silu_mul", &silu_mul);
  m.def("silu_mul_pairing", &silu_mul_pairing);
  m.def("moe_grouped_gemm", &moe_grouped_gemm);
  m.def("gemm_tile", &gemm_tile, py::arg("y"), py::arg("x"), py::arg("w"), py::arg("offsets"), py::arg("swiglu"),
        py::arg("algo") = 1, py::arg("rope_pos") = py::none(), py::arg("rope_cs") = py::none(),
        py::arg("rope_heads") = 0, py::arg("rs_part") = py::none(), py::arg("rs_eps") = 1e-5,
        py::arg("resid") = py::none(), py::arg("hw") = py::none(), py::arg("norm_w") = py::none(),
        py::arg("ss_out") = py::none(), py::arg("wscale") = py::none(), py::arg("persist") = -1, py::arg("cus") = 0);
  m.def("gemm_tile_plan", &gemm_tile_plan, py::arg("fmt"), py::arg("M"), py::arg("N"), py::arg("K"), py::arg("epi"),
        py::arg("sch"), py::arg("experts"), py::arg("rs_np"), py::arg("persist") = -1,
        py::arg("cus") = (int64_t)k8sllm::kTileCUs, py::arg("ext") = false);
  m.def("gemm_tile_forms", &gemm_tile_forms);
  m.def("gemm_tile_persist_forms", &gemm_tile_persist_forms);
  m.def("gelu_tanh", &gelu_tanh);
  m.def("embedding", &embedding);
  m.def("resolve_ids", &resolve_ids);
  m.def("rope_and_cache", &rope_and_cache);
  m.def("paged_decode", &paged_decode);
  m.def("paged_decode_fused", &paged_decode_fused);
  m.def("paged_decode_plan", &paged_decode_plan);
  m.def("paged_decode_forms", &paged_decode_forms);
  m.def("decode_tw_force", [](int64_t tw) { k8sllm_decode_tw_force((int)tw); });
  m.def("flash_prefill", &flash_prefill);
  m.def("embed_norm_partial", &embed_norm_partial);
  m.def("sample", &sample, py::arg("out"), py::arg("logits"), py::arg("temps"), py::arg("top_k"), py::arg("top_p"),
        py::arg("rng"), py::arg("advance") = false, py::arg("pen_table") = py::none(),
        py::arg("pen_params") = py::none(), py::arg("pen_slots") = py::none(), py::arg("pen_vocab") = 0,
        py::arg("g_mask") = py::none(), py::arg("g_trans") = py::none(), py::arg("g_state") = py::none(),
        py::arg("g_slots") = py::none(), py::arg("g_tok_off") = py::none(), py::arg("g_blob") = py::none(),
        py::arg("g_eos") = py::none());
  m.def("guide_mask_build", &guide_mask_build);
  m.def("penalty_reset", &penalty_reset);
  m.def("token_logprobs", &token_logprobs);
  m.def("pool_l2", &pool_l2);
  m.def("moe_route", &moe_route);
  m.def("moe_router", &moe_router);
  m.def("moe_align", &moe_align);
  m.def("moe_combine", &moe_combine);
  m.def("gather_rows", &gather_rows);
  m.def("gemm_skinny", &gemm_skinny);
  m.def("gemm_skinny_grouped", &gemm_skinny_grouped);
  m.def("gemm_skinny_forms", &gemm_skinny_forms);
  m.def("gemm_skinny_plan", &gemm_skinny_plan);
  m.def("gemm_dec_plan", &gemm_dec_plan);
  m.def("gemm_dec_plan", &gemm_dec_plan_sw);
  m.attr("SKINNY_MAX_M") = k8sllm::kSkinnyMaxM;
  m.attr("SKINNY_GROUPED_MAX_M") = k8sllm::kSkinnyGroupedMaxM;
  m.def("gemm_dec", &gemm_dec);
  m.def("gemm_dec", &gemm_dec_sw);
  m.def("gemm_dec", &gemm_dec_delta);
  m.def("gemm_dec_forms", &gemm_dec_forms);
  m.def("gemm_dec_f8_forms", &gemm_dec_f8_forms);
  m.def("gemm_dec_f4_forms", &gemm_dec_f4_forms);
  m.def("gemm_dec_rc", &gemm_dec_rc);
  m.def("reduce_add_rms_norm", &reduce_add_rms_norm);
  m.def("reduce_slabs", &reduce_slabs);
  m.def("lora_shrink_plan", &lora_shrink_plan);
  m.def("lora_shrink", &lora_shrink);
  m.def("lora_expand", &lora_expand);
  m.def("add_norm_partial", &add_norm_partial);
  m.def("car_create", &car_create);
  m.def("car_open", &car_open);
  m.def("car_all_reduce", &car_all_reduce, py::arg("state"), py::arg("in"), py::arg("out"), py::arg("spin_limit"),
        py::arg("algo") = -1);
  m.def("car_fused_tail", &car_fused_tail);
  m.def("car_all_to_all", &car_all_to_all);
  m.def("car_error", &car_error);
  m.def("car_all_gather", &car_all_gather);
  m.def("car_error_async", &car_error_async);
  m.def("car_destroy", &car_destroy);
}
