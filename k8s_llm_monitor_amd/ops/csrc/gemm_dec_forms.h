// The compiled forms of the shared-A decode GEMM (gemm_dec_kernel, gemm_decode.hip): THE table.
// k8sllm_gemm_dec dispatches by walking it and instantiates nothing else; the row limits of the
// launcher and of the bindings are derived from it; k8sllm_gemm_dec_forms reports it, and
// ops.DEC_FORMS (the Python copy dec_config picks from) is tested against that report.  Adding a
// form or a row class is one row here and the same row there.
// Plain C++: bindings.cpp (g++) includes this file, so no HIP or torch headers.
#pragma once

namespace k8sllm {

enum { DEC_SLAB = 0, DEC_BF16 = 1, DEC_SWIGLU8 = 2 };
enum { DEC_W_BF16 = 0, DEC_W_F8 = 1, DEC_W_F4 = 2 };  // the weight format of an instantiation

// One row = the instantiations <1..max_mt m-tiles, ntw, waves, epi, depth> (16 rows per m-tile:
// max_mt 4 serves <= 64 rows, 8 <= 128; above 4 the A chunks are max_mt * 8 KiB in the 2-slot LDS
// ring - 128 KiB at 8 - with max_mt x ntw accumulators per wave), and with wide_norm also the
// RNW = true ones (deferred-norm sums per 16 columns, behind gemm_dec_rc) at 1..kDecNarrowMaxMT.
struct DecForm {
  int epi, ntw, waves, depth, max_mt, wide_norm;
};

// Every Llama-3-8B / 70B / Mixtral projection and LM head at TP 1..8 lands on one of these.  The
// order is the candidate order of ops.dec_config (the first of two equal candidates wins).
constexpr DecForm kDecForms[] = {
    {DEC_SLAB, 1, 8, 8, 8, 0},      // o, down; TP 2-8 shapes
    {DEC_SLAB, 1, 6, 8, 8, 0},      // qkv: 64 groups x 4 splits (ops.DEC_TABLE only, never an automatic pick)
    {DEC_SLAB, 1, 4, 16, 4, 0},     // 70B TP=8 qkv
    {DEC_SLAB, 1, 4, 8, 8, 0},      // narrow TP shards
    {DEC_SWIGLU8, 1, 7, 8, 8, 1},   // gate_up; wide: behind the row-complete o projection
    {DEC_SWIGLU8, 1, 7, 16, 4, 1},
    {DEC_SWIGLU8, 1, 8, 16, 4, 0},  // 70B TP=1 gate_up
    {DEC_BF16, 4, 8, 4, 4, 0},      // LM head, TP=1, <= 64 rows
    {DEC_BF16, 3, 8, 8, 4, 0},
    // the head above 64 rows: 8 m-tiles x 4 n-tiles of accumulators do not fit a 2-waves-per-SIMD
    // register budget, so two n-tiles per wave
    {DEC_BF16, 2, 8, 8, 8, 0},      // vocab shards, TP 2-8
    {DEC_BF16, 1, 8, 8, 4, 0},      // Mixtral's 32000-row head
};
constexpr int kDecNForms = sizeof(kDecForms) / sizeof(kDecForms[0]);

// The rows of kDecForms that also have the fp8-weight instantiations (k8sllm_gemm_dec_f8: e4m3
// codes [N/16][K/64][64][16] plus one fp32 power-of-two scale per packed weight row; dense
// launches, narrow deferred norm, 1..max_mt m-tiles): the Llama-3-8B picks of ops.DEC_TABLE /
// DEC_TABLE_M128 and the 70B TP=1 gate_up form.  k8sllm_gemm_dec_f8_forms reports the list and
// ops.DEC_F8_FORMS mirrors it.  The SLAB and SWIGLU8 rows also serve the grouped launches over a
// quantised expert stack (k8sllm_gemm_dec_grouped_q, <= kDecNarrowMaxM rows: the same
// instantiations, the expert strides being run-time arguments); so do those of kDecF4Forms.
constexpr int kDecF8Forms[] = {0, 1, 4, 6, 7, 9};
constexpr int kDecNF8Forms = sizeof(kDecF8Forms) / sizeof(kDecF8Forms[0]);

constexpr bool dec_form_f8(int form) {
  for (int i : kDecF8Forms)
    if (i == form) return true;
  return false;
}

// The rows of kDecForms that also have the MXFP4-weight instantiations (k8sllm_gemm_dec_f4: e2m1
// codes [N/16][K/128][64][16] plus the e8m0 block scales [N/16][K/128][16] dwords; dense launches,
// narrow deferred norm, 1..max_mt m-tiles): every pick of ops.DEC_TABLE / DEC_TABLE_M128.  The F4
// ring depth (k-steps in flight per n-tile, four per load) replaces the row's own: 8 at every row
// count, and at one m-tile (<= 16 rows) the `depth` given here where it divides the K slice's
// k-steps - 16 measured 1-4 % faster than 8 at 1 row and 3-10 % slower at 64 and 128; 32 gained
// nothing and spills at 8 m-tiles (profiles/r13/README.md).  A slice need only hold whole 256-deep
// A chunks.  Four n-tiles per wave stay at 8 (16 spills at 4 m-tiles and was not tried at one).
// k8sllm_gemm_dec_f4_forms reports the list and ops.DEC_F4_FORMS mirrors it.
struct DecF4Form {
  int form, depth;
};
constexpr DecF4Form kDecF4Forms[] = {{0, 16}, {1, 16}, {4, 16}, {7, 8}, {9, 16}};
constexpr int kDecNF4Forms = sizeof(kDecF4Forms) / sizeof(kDecF4Forms[0]);

constexpr int dec_form_f4_depth(int form) {  // the row's F4 ring depth at one m-tile; 0: no mxfp4 instantiation
  for (const DecF4Form& f : kDecF4Forms)
    if (f.form == form) return f.depth;
  return 0;
}

constexpr int dec_max_mt() {
  int m = 0;
  for (const DecForm& f : kDecForms) m = f.max_mt > m ? f.max_mt : m;
  return m;
}

// Row limits: dense launches up to the largest form; grouped launches (experts > 1 or routing
// weights), the wide deferred-norm form and the row-complete kernel stay at 4 m-tiles.
constexpr int kDecNarrowMaxMT = 4;
constexpr int kDecMaxM = 16 * dec_max_mt();        // 128
constexpr int kDecNarrowMaxM = 16 * kDecNarrowMaxMT;  // 64

}  // namespace k8sllm
