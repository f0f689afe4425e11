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

// The rows of kDecForms that also have the fp8-weight instantiations (wf = DEC_W_F8: e4m3
// codes [N/16][K/64][64][16] plus one fp32 power-of-two scale per packed weight row; dense
// launches, narrow deferred norm, 1..max_mt m-tiles): the Llama-3-8B picks of ops.DEC_TABLE /
// DEC_TABLE_M128 and the 70B TP=1 gate_up form.  k8sllm_gemm_dec_f8_forms reports the list and
// ops.DEC_F8_FORMS mirrors it.  The SLAB and SWIGLU8 rows also serve the grouped launches over a
// quantised expert stack (experts >= 1, <= kDecNarrowMaxM rows: the same
// instantiations, the expert strides being run-time arguments); so do those of kDecF4Forms.
constexpr int kDecF8Forms[] = {0, 1, 4, 6, 7, 9};
constexpr int kDecNF8Forms = sizeof(kDecF8Forms) / sizeof(kDecF8Forms[0]);

constexpr bool dec_form_f8(int form) {
  for (int i : kDecF8Forms)
    if (i == form) return true;
  return false;
}

// The rows of kDecForms that also have the MXFP4-weight instantiations (wf = DEC_W_F4: e2m1
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

// Row limits: dense launches up to the largest form; grouped launches (an expert stack or routing
// weights), the wide deferred-norm form and the row-complete kernel stay at 4 m-tiles.
constexpr int kDecNarrowMaxMT = 4;
constexpr int kDecMaxM = 16 * dec_max_mt();        // 128
constexpr int kDecNarrowMaxM = 16 * kDecNarrowMaxMT;  // 64

// Kernel constants the plan needs (gemm_decode.hip asserts they are the kernel's own).
constexpr int kDecAChunk = 8;     // kDecCH: k-steps (32 deep) per A chunk in the LDS ring
constexpr int kDecRnNarrow = 16;  // 4 * kRnMax: deferred-norm partial sums per row of the narrow form
constexpr int kDecRnWide = 256;   // 16 * kRnWide: of the wide form (a multiple of 16)

// What one launch of gemm_dec_kernel does.  err: 0, or -1 arguments / limits, -3 K slicing, -4
// splits with a non-slab epilogue, -5 no such form (nothing else is then meaningful but max_m).
struct DecPlan {
  int err;
  int max_m;       // the row limit of this kind of launch (kDecMaxM or kDecNarrowMaxM)
  int mt;          // m-tiles
  int kchunk;      // K per split
  int d4;          // mxfp4: the ring depth in k-steps (8 or 16), else 0
  int rnw;         // 1: the wide deferred-norm instantiation
  int gx, gy, gz;  // grid: column groups, splits, experts
  int slabs;       // what the caller is told: fp32 slabs written (SLAB), else 1
  int rows;        // SLAB: the row-wide 16-byte slab stores (else one float per lane)
  int wt;          // SLAB: those stores write through (sc1); only with rows
  int xcd;         // SLAB: one split per XCD (dec_xcd_map), else the identity map
};

// The kernel's flags argument: the three fields above.
enum { kDecRows = 1, kDecWt = 2, kDecXcd = 4 };

// One split per XCD.  Workgroups are observed to be dealt round-robin over the 8 XCDs, so the
// linear ids L = x + gx * y with equal L % 8 share an L2.  For `splits` in {2, 4, 8} and gx * splits
// a multiple of 8: XCD c = L % 8 takes split c % splits, and its j-th workgroup (j = L / 8) takes
// column group j * (8 / splits) + c / splits - a bijection onto [0, gx) x [0, splits), so every
// workgroup of the plain grid is still run exactly once wherever the dispatcher puts it.
// ops.dec_xcd_map is the Python copy (tests/test_dec_slab_plan_cpu.py).
struct DecXY {
  int x, y;
};
constexpr bool dec_xcd_ok(int gx, int splits) {
  return (splits == 2 || splits == 4 || splits == 8) && (gx * splits) % 8 == 0;
}
constexpr DecXY dec_xcd_map(int L, int splits) {
  const int c = L & 7, j = L >> 3, per = 8 / splits;
  return DecXY{j * per + c / splits, c % splits};
}

// The row of kDecForms that is (epi, ntw, waves, depth), or -1.
constexpr int dec_form_index(int epi, int ntw, int waves, int depth) {
  for (int i = 0; i < kDecNForms; ++i) {
    const DecForm& f = kDecForms[i];
    if (f.epi == epi && f.ntw == ntw && f.waves == waves && f.depth == depth) return i;
  }
  return -1;
}

// What ships (switch -1) for a SLAB launch of M rows: by row class, from the A/B of
// profiles/r24/README.md.  Above one m-tile everything is on (64 rows: qkv 12.7 -> 11.5 us, o
// 10.2 -> 9.2, down 22.9 -> 21.7).  At one m-tile the row-wide stores do not pay (0.2 us slower at 1
// row; they are not compiled there) and only the placement stays (o 7.45 -> 7.2 us at 1 row, qkv
// 10.5 -> 10.35 at 16).  ops.dec_slab_shipped mirrors it.
struct DecSlabSw {
  int rows, wt, xcd;
};
constexpr DecSlabSw dec_slab_shipped(int M) {
  const int wide = M > 16;
  return DecSlabSw{wide, wide, 1};
}

// THE plan of k8sllm_gemm_dec: the launcher, the binding (its row limit and slab count) and the
// CPU tests (native().gemm_dec_plan against ops.dec_form_ok) all take their answers from here.
// wf: DEC_W_*; experts: 0 a dense launch, E >= 1 a grouped one over an [E, ...] stack (grid.z =
// expert); has_row_w: routing weights scale the slabs; rn_nc: deferred-norm partial sums per A row
// (0: no deferred norm); f4_depth: mxfp4 ring depth, 0 = the rule below, 8 / 16 forced within it.
//
// Accepted launches (everything else is refused):
//
//   weights  launch   rows     K %   epilogues            deferred norm      forms (1..max_mt m-tiles)
//   bf16     dense    <= 128   32    SLAB BF16 SWIGLU8    narrow, or wide    kDecForms; wide: its wide_norm
//                                                         at <= 64 rows      rows at 1..4 m-tiles
//   bf16     grouped  <= 64    32    SLAB BF16 SWIGLU8    as dense (the      as dense
//                                                         binding gives none)
//   fp8      dense    <= 128   64    SLAB BF16 SWIGLU8    narrow             kDecF8Forms
//   mxfp4    dense    <= 128   128   SLAB BF16 SWIGLU8    narrow             kDecF4Forms
//   fp8      grouped  <= 64    64    SLAB SWIGLU8         none               kDecF8Forms
//   mxfp4    grouped  <= 64    128   SLAB SWIGLU8         none               kDecF4Forms
//
// Every one: N % 16 == 0, splits >= 1 dividing K, splits == 1 unless SLAB, routing weights only
// with SLAB (and they make a launch grouped).  K slices: bf16 / fp8 a positive multiple of
// max(depth, kDecAChunk) k-steps (one unrolled main-loop iteration); mxfp4 whole 256-deep A chunks,
// and the ring depth d4 dividing the slice's k-steps: the kDecF4Forms row's depth at one m-tile,
// 8 above, and 0 -> the deepest of those that divides.
//
// sw_rows, sw_wt, sw_xcd: the A/B switches ops.DEC_SLAB_ROWS, DEC_SLAB_WT and DEC_XCD_SPLITS: 1 on
// wherever the launch can take it, 0 off, -1 as shipped (dec_slab_shipped).  SLAB launches only:
// rows at two m-tiles and up (the one-m-tile kernels do not hold that path) where a slab stays under
// 2 GiB (32-bit buffer offsets), wt only with rows, xcd on dense launches that dec_xcd_ok accepts.
constexpr DecPlan dec_plan(int wf, int M, int N, int K, int splits, int epi, int ntw, int waves, int depth,
                           int f4_depth, int experts, bool has_row_w, int rn_nc, int sw_rows = -1, int sw_wt = -1,
                           int sw_xcd = -1) {
  DecPlan p{-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const bool grouped = experts >= 1 || has_row_w, quant = wf != DEC_W_BF16;
  p.max_m = grouped ? kDecNarrowMaxM : kDecMaxM;
  if ((wf != DEC_W_BF16 && wf != DEC_W_F8 && wf != DEC_W_F4) || experts < 0 || M < 1 || M > p.max_m) return p;
  if (has_row_w && epi != DEC_SLAB) return p;
  if (quant && grouped && ((epi != DEC_SLAB && epi != DEC_SWIGLU8) || rn_nc > 0)) return p;
  if (N % 16 || K % (wf == DEC_W_F4 ? 128 : wf == DEC_W_F8 ? 64 : 32) || splits < 1 || K % splits) return p;
  const int form = dec_form_index(epi, ntw, waves, depth);
  if (ntw * waves < 1 || (wf == DEC_W_F4 && (form < 0 || dec_form_f4_depth(form) == 0))) return p.err = -5, p;
  p.mt = (M + 15) / 16;
  p.kchunk = K / splits;
  const int ks = p.kchunk / 32;  // k-steps per slice
  p.err = -3;
  if (wf == DEC_W_F4) {
    if (p.kchunk % 128 || ks < kDecAChunk || ks % kDecAChunk) return p;
    const int dmax = p.mt > 1 ? 8 : dec_form_f4_depth(form);
    p.d4 = f4_depth ? f4_depth : dmax >= 16 && ks % 16 == 0 ? 16 : 8;
    if ((p.d4 != 8 && p.d4 != 16) || p.d4 > dmax || ks % p.d4) return p;
  } else {
    const int iter = depth > kDecAChunk ? depth : kDecAChunk;
    if (p.kchunk % 32 || ks < iter || ks % iter) return p;
  }
  if (epi != DEC_SLAB && splits != 1) return p.err = -4, p;
  p.rnw = rn_nc > kDecRnNarrow;
  // the wide deferred-norm form (gemm_dec_rc's sums) reads bf16 weights
  if (p.rnw && (quant || rn_nc % 16 || rn_nc > kDecRnWide)) return p.err = -1, p;
  // the m-tile counts the row is instantiated with for this request: dec_dispatch's conditions
  int max_mt = 0;
  if (form >= 0) {
    const DecForm& f = kDecForms[form];
    if (wf == DEC_W_F8) max_mt = dec_form_f8(form) ? f.max_mt : 0;
    else if (wf == DEC_W_F4) max_mt = p.d4 == 16 ? 1 : f.max_mt;
    else max_mt = p.rnw ? (f.wide_norm ? kDecNarrowMaxMT : 0) : f.max_mt;
  }
  if (p.mt > max_mt) return p.err = -5, p;
  const int nwg = ntw * waves;
  p.gx = (N / 16 + nwg - 1) / nwg;
  p.gy = splits;
  p.gz = experts > 1 ? experts : 1;
  p.slabs = epi == DEC_SLAB ? p.gz * splits : 1;
  if (epi == DEC_SLAB) {
    const DecSlabSw d = dec_slab_shipped(M);
    p.rows = (sw_rows < 0 ? d.rows : sw_rows) != 0 && p.mt > 1 && (long)M * N * 4 < 0x7fffffffL;
    p.wt = p.rows && (sw_wt < 0 ? d.wt : sw_wt) != 0;
    p.xcd = (sw_xcd < 0 ? d.xcd : sw_xcd) != 0 && !grouped && dec_xcd_ok(p.gx, splits);
  }
  p.err = 0;
  return p;
}

}  // namespace k8sllm
