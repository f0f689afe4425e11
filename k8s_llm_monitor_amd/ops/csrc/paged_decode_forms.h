// The compiled forms of paged decode attention (paged_decode_kernel, paged_decode.hip): THE table,
// and the plan of one launch.  k8sllm_paged_decode dispatches by walking the table and instantiates
// nothing else; the binding takes every rule that depends on numbers from pd_plan;
// k8sllm_paged_decode_forms reports the table, and ops.PD_FORMS (the Python copy that
// ops.paged_decode_why answers from) is tested against that report.  Adding a form is one row here
// and the same row there.
// Plain C++: bindings.cpp (g++) includes this file, so no HIP or torch headers.
#pragma once

namespace k8sllm {

constexpr int kBS = 16;            // tokens per KV-cache block
constexpr int kPdMaxSplits = 64;   // splits per (sequence, kv head): one lane per split in the merge (ops.MAX_SPLITS)
// Tokens per wave per chunk (TW), measured on MI355X (tools/bench_decode.py, bench_decode_step.py):
// TW = 32, two chunk buffers per wave (double-buffered loads, ~240 VGPRs: 2 waves per SIMD), once the
// grid fills the chip - from kPdTw32MinWg workgroups on, e.g. batch 64 x 8 kv heads = 512; below that
// TW = 64, one buffer of 64 tokens (~120 VGPRs: up to 4 workgroups per CU), for small batches and
// split grids, where residency, not the per-wave pipeline, hides the memory latency.
constexpr int kPdTw32MinWg = 384;

// One row = head dim D, G = Hq / Hkv query heads per KV head, fused (FQ: the qkv slab reduce, RoPE and
// the KV write in the attention kernel), f8 (an e4m3 cache).  A row stands for its TW = 32 and
// TW = 64 instantiations, a fused row also for MERGE false and true (the in-launch merge of the
// split partials): 14 x 2 + 8 x 4 = 60 kernels, and one reduce kernel per unfused bf16 row (9).
struct PdForm {
  int D, G, fused, f8;
};

constexpr PdForm kPdForms[] = {
    {128, 1, 0, 0}, {128, 2, 0, 0}, {128, 4, 0, 0}, {128, 8, 0, 0}, {128, 16, 0, 0},
    {64, 1, 0, 0},  {64, 2, 0, 0},  {64, 4, 0, 0},  {64, 8, 0, 0},
    {128, 1, 0, 1}, {128, 2, 0, 1}, {128, 4, 0, 1}, {128, 8, 0, 1}, {128, 16, 0, 1},
    // fused: no G = 16 (a D = 128 model with 16 query heads per KV head decodes unfused)
    {128, 1, 1, 0}, {128, 2, 1, 0}, {128, 4, 1, 0}, {128, 8, 1, 0},
    {128, 1, 1, 1}, {128, 2, 1, 1}, {128, 4, 1, 1}, {128, 8, 1, 1},
};
constexpr int kPdNForms = sizeof(kPdForms) / sizeof(kPdForms[0]);

// The row of kPdForms that is (D, G, fused, f8), or -1.
constexpr int pd_form_index(int D, int G, bool fused, bool f8) {
  for (int i = 0; i < kPdNForms; ++i) {
    const PdForm& f = kPdForms[i];
    if (f.D == D && f.G == G && (f.fused != 0) == fused && (f.f8 != 0) == f8) return i;
  }
  return -1;
}

// What one launch of k8sllm_paged_decode does.  err: 0, or -1 no such form, -2 splits, -3 arguments
// (nothing else is then meaningful).
struct PdPlan {
  int err;
  int form;        // the row of kPdForms
  int tw;          // tokens per wave per chunk: 32 or 64
  int merge;       // the split partials are merged inside the launch by the last-arriving split
  int reduce;      // ... or by a paged_decode_reduce_kernel launch, grid (Hkv, B)
  int gx, gy, gz;  // the grid: (S, Hkv, B)
};

// THE plan of k8sllm_paged_decode: the launcher, the binding and the CPU tests
// (native().paged_decode_plan against ops.paged_decode_why) all take their answers from here.
// S: splits per (sequence, kv head), the caller's choice (ops.decode_splits); merge_wanted: the
// caller passed merge counters; tw_force: 32 / 64 forces one TW (tools), anything else: by grid size.
//
// B <= 0 is an empty launch of any form: err 0, nothing planned.  The order of the checks decides
// the code of a doubly-wrong request: -2 (S outside [1, kPdMaxSplits]) before -3 (an e4m3 cache or
// the fused form with D != 128) before -1 (no row for (D, G, fused, f8); G = Hq / Hkv).
constexpr PdPlan pd_plan(int D, int Hq, int Hkv, int B, int S, bool fused, bool f8, bool merge_wanted, int tw_force) {
  PdPlan p{0, -1, 0, 0, 0, 0, 0, 0};
  if (B <= 0) return p;
  if (S < 1 || S > kPdMaxSplits) return p.err = -2, p;
  if ((f8 || fused) && D != 128) return p.err = -3, p;
  p.form = Hkv > 0 ? pd_form_index(D, Hq / Hkv, fused, f8) : -1;
  if (p.form < 0) return p.err = -1, p;
  p.tw = tw_force == 32 || tw_force == 64 ? tw_force : (long)S * Hkv * B >= kPdTw32MinWg ? 32 : 64;
  p.merge = fused && merge_wanted && S > 1;
  p.reduce = S > 1 && !p.merge;
  p.gx = S, p.gy = Hkv, p.gz = B;
  return p;
}

}  // namespace k8sllm
