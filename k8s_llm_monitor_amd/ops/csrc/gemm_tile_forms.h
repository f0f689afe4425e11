// The compiled forms of the 256 x 256 prefill tile GEMM (gemm_w4_kernel, gemm_tile.hip): THE table,
// and the plan of one launch.  k8sllm_gemm_tile dispatches by walking the table and instantiates
// nothing else; the binding takes every rule that depends on numbers from tile_plan;
// k8sllm_gemm_tile_forms reports the table, and ops.TILE_FORMS (the Python copy the CPU path checks
// against) is tested against that report.  Adding a form is one row here and the same row there.
// Plain C++: bindings.cpp (g++) includes this file, so no HIP or torch headers.
#pragma once

namespace k8sllm {

enum { TILE_EPI_BF16 = 0, TILE_EPI_SWIGLU = 1, TILE_EPI_ROPE = 2, TILE_EPI_RESID = 3, TILE_EPI_SWIGLU8 = 4 };
enum { TILE_W_BF16 = 0, TILE_W_F8 = 1, TILE_W_F4 = 2 };  // the weight format of an instantiation

// What a weight format asks of K (always whole 64-deep k-tiles): at least min_k, and whole k_group-deep
// scale groups (0: the format has none along K); bits per weight, for the 32-bit DMA offsets.
struct TileFmt {
  int min_k, k_group, bits;
};
constexpr TileFmt kTileFmts[] = {
    {64, 0, 16},   // bf16, row-major or fragment-packed (wpk is a run-time argument)
    {192, 0, 8},   // fp8: schedule 1 only, whose peeled ring tail needs three k-tiles
    {256, 128, 4}, // mxfp4: a code block and its e8m0 scales span two k-tiles
};
constexpr int kTileNFmts = sizeof(kTileFmts) / sizeof(kTileFmts[0]);

// One row = the instantiation <epi, grouped, SCH 1, rs, fmt> and, with sch0, its SCH 0 twin.
struct TileForm {
  int fmt, epi, grouped, rs, sch0;
};

constexpr TileForm kTileForms[] = {
    {TILE_W_BF16, TILE_EPI_BF16, 0, 0, 1},
    {TILE_W_BF16, TILE_EPI_SWIGLU, 0, 0, 1},
    {TILE_W_BF16, TILE_EPI_SWIGLU8, 0, 0, 1},
    {TILE_W_BF16, TILE_EPI_ROPE, 0, 0, 1},
    {TILE_W_BF16, TILE_EPI_RESID, 0, 0, 0},  // the fused-norm producers and consumers: schedule 1
    {TILE_W_BF16, TILE_EPI_SWIGLU, 0, 1, 0},
    {TILE_W_BF16, TILE_EPI_SWIGLU8, 0, 1, 0},
    {TILE_W_BF16, TILE_EPI_ROPE, 0, 1, 0},
    {TILE_W_BF16, TILE_EPI_BF16, 1, 0, 1},  // the expert GEMMs
    {TILE_W_BF16, TILE_EPI_SWIGLU, 1, 0, 1},
    {TILE_W_BF16, TILE_EPI_SWIGLU8, 1, 0, 1},
    // the codes a packed dense layer keeps: what its prefill launches, and no other schedule
    {TILE_W_F8, TILE_EPI_BF16, 0, 0, 0},
    {TILE_W_F8, TILE_EPI_SWIGLU8, 0, 0, 0},
    {TILE_W_F8, TILE_EPI_SWIGLU8, 0, 1, 0},
    {TILE_W_F8, TILE_EPI_ROPE, 0, 0, 0},
    {TILE_W_F8, TILE_EPI_ROPE, 0, 1, 0},
    {TILE_W_F8, TILE_EPI_RESID, 0, 0, 0},
    {TILE_W_F4, TILE_EPI_BF16, 0, 0, 0},
    {TILE_W_F4, TILE_EPI_SWIGLU8, 0, 0, 0},
    {TILE_W_F4, TILE_EPI_SWIGLU8, 0, 1, 0},
    {TILE_W_F4, TILE_EPI_ROPE, 0, 0, 0},
    {TILE_W_F4, TILE_EPI_ROPE, 0, 1, 0},
    {TILE_W_F4, TILE_EPI_RESID, 0, 0, 0},
};
constexpr int kTileNForms = sizeof(kTileForms) / sizeof(kTileForms[0]);

// The persistent instantiations, beside the table: the dense bf16 schedule-1 rows (epi, rs) that are
// ALSO compiled with PERSIST (a grid of min(tiles, CUs) workgroups that walk the tiles, the next
// tile's ring fill overlapping the epilogue: gemm_tile.hip) - the launches of the fused-norm prefill
// layer.  on: tile_plan routes the row there by itself (measured faster: profiles/r23/README.md);
// 0: only when forced.  ops.TILE_PERSIST_FORMS is the Python copy (tests/test_tile_persist_cpu.py).
struct TilePersistForm {
  int epi, rs, on;
};
constexpr TilePersistForm kTilePersist[] = {
    {TILE_EPI_ROPE, 1, 1},     // qkv: RoPE + row scale
    {TILE_EPI_RESID, 0, 1},    // o, down: residual add + the next norm's operands
    {TILE_EPI_SWIGLU8, 1, 1},  // gate_up: SwiGLU (per-16 pairing) + row scale
};
constexpr int kTileNPersist = sizeof(kTilePersist) / sizeof(kTilePersist[0]);
constexpr int kTileCUs = 256;  // MI355X; the launcher plans with the device's own count

// The row of kTilePersist that is (epi, rs), or -1.
constexpr int tile_persist_index(int epi, bool rs) {
  for (int i = 0; i < kTileNPersist; ++i)
    if (kTilePersist[i].epi == epi && (kTilePersist[i].rs != 0) == rs) return i;
  return -1;
}

constexpr int kTileMaxExperts = 256;  // grouped: the kernel walks the offsets of every expert per workgroup
constexpr int kTileSch1MinK = 192;    // schedule 1's peeled ring tail needs three k-tiles
constexpr int kTileRsMaxNp = 64;      // row scale: the kernel loads a fixed 16 x 4 partial sums per row

// The row of kTileForms that is (fmt, epi, grouped, rs), or -1.
constexpr int tile_form_index(int fmt, int epi, bool grouped, bool rs) {
  for (int i = 0; i < kTileNForms; ++i) {
    const TileForm& f = kTileForms[i];
    if (f.fmt == fmt && f.epi == epi && (f.grouped != 0) == grouped && (f.rs != 0) == rs) return i;
  }
  return -1;
}

constexpr bool tile_fmt_has_epi(int fmt, int epi) {
  for (const TileForm& f : kTileForms)
    if (f.fmt == fmt && f.epi == epi) return true;
  return false;
}

// tile_plan's E / rs_np for a launch that has offsets / row-scale partial sums (`present`) and n
// experts / partials per row: present with none is an argument the plan refuses.
constexpr int tile_count_arg(bool present, int n) { return !present ? 0 : n != 0 ? n : -1; }

// What one launch of gemm_w4_kernel does.  err: 0, or -1 arguments, -2 grid, -3 32-bit offsets, -4 no
// such quantised form (nothing else is then meaningful).
struct TilePlan {
  int err;
  int sch;         // the schedule that runs (0 or 1)
  int form;        // the row of kTileForms
  int n_mt, n_nt;  // m-tiles (grouped: ceil(M / 256) + E, the bound over any split of the rows), n-tiles
  int nwg;         // tiles: n_mt * n_nt
  int persist;     // the row of kTilePersist that runs, or -1: the one-tile form, one workgroup per tile
  int grid;        // workgroups launched: nwg, or min(nwg, CUs) for a persistent launch
};

// THE plan of k8sllm_gemm_tile: the launcher, the binding and the CPU tests (native().gemm_tile_plan
// against ops.tile_form_why) all take their answers from here.  fmt: TILE_W_*; sch: the requested
// schedule; E: 0 a dense launch, else a grouped one over E experts; rs_np: row-scale partial sums
// per row, 0 = no row scale (tile_count_arg makes both).
//
// Accepted launches (everything else is refused):
//
//   weights  launch           K                    epilogues (+RS: also with the row scale)      schedules
//   bf16     dense            >= 64                BF16 SWIGLU+RS SWIGLU8+RS ROPE+RS             0, 1; +RS: 1
//   bf16     dense            >= 192               RESID                                         1
//   bf16     grouped, E<=256  >= 64                BF16 SWIGLU SWIGLU8                           0, 1
//   fp8      dense            >= 192               BF16 SWIGLU8+RS ROPE+RS RESID                 1
//   mxfp4    dense            >= 256, % 128 == 0   BF16 SWIGLU8+RS ROPE+RS RESID                 1
//
// Every one: N % 16 == 0, K % 64 == 0; SWIGLU / SWIGLU8 N % 256 == 0; ROPE / RESID N % 128 == 0;
// RS 4 <= rs_np <= 64, rs_np % 4 == 0.  bf16 below K = 192: a schedule-1 request runs schedule 0
// where the row has it (RESID and RS have not: refused).  32-bit DMA offsets: the weight (one
// expert's), 256 rows of X and, for RESID, 256 rows of the residual stay below 2^31 bytes; at most
// 2^30 workgroups.  M <= 0 is an empty launch of any form: err 0, nothing planned.
//
// The order of the checks decides the code of a doubly-wrong request: -4 (a quantised W asked for
// a form its format does not have) before -1 before -3 before -2.
//
// Persistent or not: a dense bf16 schedule-1 launch whose (epi, rs) is a row of kTilePersist and that
// has more tiles than the device has CUs (`cus`; up to one tile per CU the one-tile form is the same
// launch) runs persistent where the row is `on`.  `persist` overrides the rows' `on` for A/B runs: 1
// every such launch, 0 none, -1 (the default) as the table says.  Everything else - grouped, fp8 /
// mxfp4, schedule 0, rows not in the table - is the one-tile form whatever is asked.
constexpr TilePlan tile_plan(int fmt, int M, int N, int K, int epi, int sch, int E, int rs_np, int persist = -1,
                             int cus = kTileCUs) {
  TilePlan p{-4, 0, -1, 0, 0, 0, -1, 0};
  if (fmt < 0 || fmt >= kTileNFmts) return p;
  if (M <= 0) return p.err = 0, p;
  const TileFmt& f = kTileFmts[fmt];
  const bool grouped = E != 0, rs = rs_np != 0, epi_ok = epi >= TILE_EPI_BF16 && epi <= TILE_EPI_SWIGLU8;
  if (fmt != TILE_W_BF16 && (grouped || sch != 1 || K < f.min_k || (f.k_group && K % f.k_group) ||
                             (epi_ok && !tile_fmt_has_epi(fmt, epi))))
    return p;
  p.err = -1;
  if (E < 0 || E > kTileMaxExperts || sch < 0 || sch > 1) return p;
  if (sch == 1 && K < kTileSch1MinK) sch = 0;  // bf16 only; a row without schedule 0 is refused below
  const bool swg = epi == TILE_EPI_SWIGLU || epi == TILE_EPI_SWIGLU8;
  if (N % 16 || K % 64 || K < f.min_k || (swg && N % 256)) return p;
  if ((epi == TILE_EPI_ROPE || epi == TILE_EPI_RESID) && N % 128) return p;
  if (rs && (rs_np < 4 || rs_np > kTileRsMaxNp || rs_np % 4)) return p;
  // dense-only ROPE / RESID / RS, RS only with SWIGLU / SWIGLU8 / ROPE, epi out of range: no row
  p.form = tile_form_index(fmt, epi, grouped, rs);
  if (p.form < 0 || (sch == 0 && !kTileForms[p.form].sch0)) return p;
  p.sch = sch;
  p.err = -3;
  if ((long)N * K / 8 * f.bits >= (1L << 31) || 256L * K * 2 >= (1L << 31)) return p;
  if (epi == TILE_EPI_RESID && 256L * N * 2 >= (1L << 31)) return p;
  p.n_mt = M / 256 + (M % 256 != 0) + E;
  p.n_nt = N / 256 + (N % 256 != 0);
  if ((long)p.n_mt * p.n_nt > (1L << 30)) return p.err = -2, p;
  p.nwg = p.grid = p.n_mt * p.n_nt;
  p.err = 0;
  const int pi = fmt == TILE_W_BF16 && !grouped && sch == 1 ? tile_persist_index(epi, rs) : -1;
  if (pi >= 0 && cus > 0 && p.nwg > cus && (persist < 0 ? kTilePersist[pi].on != 0 : persist != 0)) {
    p.persist = pi;
    p.grid = cus;
  }
  return p;
}

}  // namespace k8sllm
