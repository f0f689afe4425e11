// The host side of the skinny decode GEMM (gemm_skinny.hip) in one place: the compiled forms
// (kSkinnyForms: k8sllm_gemm_skinny dispatches by walking it and instantiates nothing else), the
// row limits, the split-K slicing rule and skinny_plan - every decision of a launch.  The bindings
// take the limits, the error decision and the slab count they report from skinny_plan as well, so
// what a caller is told is what the kernel writes.  ops/__init__.py mirrors the limits and the
// slicing rule for the CPU path; tests/test_skinny_pack.py compares the mirrors with this file.
// Plain C++: bindings.cpp (g++) includes this file, so no HIP or torch headers.
#pragma once

namespace k8sllm {

enum { EPI_SLAB = 0, EPI_BF16 = 1, EPI_SWIGLU = 2, EPI_SWIGLU_PACKED = 3 };

// PACKED: gemm_skinny_kernel over the fragment-packed weight; RM: gemm_skinny_rm_kernel over the
// row-major [N][K] weight (always with a fragment-packed A).
enum { SKINNY_PACKED = 0, SKINNY_RM = 1 };

// Row limits: 4 m-tiles of 16 rows; 8 for grouped (expert) launches over row-major weights.
constexpr int kSkinnyMaxM = 64;
constexpr int kSkinnyGroupedMaxM = 128;

// One row = the instantiations <min_mt..max_mt m-tiles, nt n-tiles, epi, a_packed, waves> of the
// family's kernel (a_packed is no template argument of the RM kernel).
struct SkinnyForm {
  int family, epi, nt, waves, a_packed, min_mt, max_mt;
};

constexpr SkinnyForm kSkinnyForms[] = {
    {SKINNY_PACKED, EPI_SLAB, 2, 4, 0, 1, 4},          {SKINNY_PACKED, EPI_SLAB, 2, 4, 1, 1, 4},
    {SKINNY_PACKED, EPI_SLAB, 2, 8, 0, 1, 4},          {SKINNY_PACKED, EPI_SLAB, 2, 8, 1, 1, 4},
    {SKINNY_PACKED, EPI_SLAB, 4, 4, 0, 1, 4},          {SKINNY_PACKED, EPI_SLAB, 4, 4, 1, 1, 4},
    {SKINNY_PACKED, EPI_SLAB, 4, 8, 0, 1, 4},          {SKINNY_PACKED, EPI_SLAB, 4, 8, 1, 1, 4},
    {SKINNY_PACKED, EPI_BF16, 2, 4, 0, 1, 4},          {SKINNY_PACKED, EPI_BF16, 2, 4, 1, 1, 4},
    {SKINNY_PACKED, EPI_BF16, 2, 8, 0, 1, 4},          {SKINNY_PACKED, EPI_BF16, 2, 8, 1, 1, 4},
    {SKINNY_PACKED, EPI_BF16, 4, 4, 0, 1, 4},          {SKINNY_PACKED, EPI_BF16, 4, 4, 1, 1, 4},
    {SKINNY_PACKED, EPI_BF16, 4, 8, 0, 1, 4},          {SKINNY_PACKED, EPI_BF16, 4, 8, 1, 1, 4},
    {SKINNY_PACKED, EPI_SWIGLU, 4, 4, 0, 1, 4},        {SKINNY_PACKED, EPI_SWIGLU, 4, 4, 1, 1, 4},
    {SKINNY_PACKED, EPI_SWIGLU, 4, 8, 0, 1, 4},        {SKINNY_PACKED, EPI_SWIGLU, 4, 8, 1, 1, 4},
    {SKINNY_PACKED, EPI_SWIGLU_PACKED, 4, 4, 0, 1, 4}, {SKINNY_PACKED, EPI_SWIGLU_PACKED, 4, 4, 1, 1, 4},
    {SKINNY_PACKED, EPI_SWIGLU_PACKED, 4, 8, 0, 1, 4}, {SKINNY_PACKED, EPI_SWIGLU_PACKED, 4, 8, 1, 1, 4},
    {SKINNY_RM, EPI_SLAB, 4, 2, 1, 1, 4},              {SKINNY_RM, EPI_SLAB, 4, 4, 1, 1, 4},
    {SKINNY_RM, EPI_BF16, 4, 2, 1, 1, 4},              {SKINNY_RM, EPI_BF16, 4, 4, 1, 1, 4},
    {SKINNY_RM, EPI_SWIGLU, 4, 2, 1, 1, 4},            {SKINNY_RM, EPI_SWIGLU, 4, 4, 1, 1, 4},
    {SKINNY_RM, EPI_SWIGLU_PACKED, 4, 2, 1, 1, 4},     {SKINNY_RM, EPI_SWIGLU_PACKED, 4, 4, 1, 1, 4},
    {SKINNY_RM, EPI_SLAB, 3, 4, 1, 1, 4},  // 48-column tiles (qkv)
    // 65..128 rows of a grouped launch: 8 m-tiles of A per stage, so 2-wave workgroups
    {SKINNY_RM, EPI_SLAB, 4, 2, 1, 5, 8},              {SKINNY_RM, EPI_SWIGLU_PACKED, 4, 2, 1, 5, 8},
};
constexpr int kSkinnyNForms = sizeof(kSkinnyForms) / sizeof(kSkinnyForms[0]);

// LDS layout of gemm_skinny_rm_kernel: per wave a ring of two stages (W tile + MT A fragments, 64 k
// deep), aliased after the main loop by the cross-wave combine.
template <int MT, int NT, int EPI, int WAVES>
struct SkinnyRmGeom {
  static constexpr int U = 2;                        // k-steps per stage: 64 k = one 128-B line per row
  static constexpr int WB = NT * 16 * 128;           // W bytes per stage
  static constexpr int AB = MT * U * 1024;           // A bytes per stage
  static constexpr int SB = WB + AB;
  static constexpr int RING = 2 * SB;                // per wave
  static constexpr int LDR = NT * 16 + 4;            // combine row pitch (floats): conflict-free
  static constexpr int RED = WAVES * MT * 16 * LDR * 4;  // cross-wave combine (aliases the rings)
  static constexpr int EPI_LDS = RED + MT * 16 * 4;  // + s_inv, written after the main loop
  static constexpr int LDS = WAVES * RING > EPI_LDS ? WAVES * RING : EPI_LDS;
  static constexpr int NLOAD = NT * 2 + MT * U;      // DMA instructions per stage
};

// kchunk: K split into `S` slices rounded up to whole wave groups (128 k) where that keeps the
// slice count, else to whole granules.
// `gran`: the smallest slice granule (32: one k-step; 64 for the row-major kernel's 64-deep stages).
constexpr int skinny_kchunk(int K, int S, int gran) {
  int kc = (K + S - 1) / S;
  const int kc128 = (kc + 127) / 128 * 128;
  if ((K + kc128 - 1) / kc128 == S) return kc128;
  return (kc + gran - 1) / gran * gran;
}

// Automatic split-K - the largest power of two that keeps the grid within one workgroup per CU,
// K slices >= 512 deep and whole 256-deep rounds of the 4 waves (uneven rounds leave waves idle at
// the tail).  Measured at M = 64 (tools/bench_skinny_waves.py,
// profiles/r01_s3_skinny_waves.jsonl): qkv S 2 14.9 us vs S 3 18.1 us; o / down S 4 beat 2, 3, 6
// and 8.  (A 128-column variant for 32 < M <= 64 measured 10-25 % slower and was removed.)
constexpr int skinny_auto_splits(int M, int N, int K) {
  const int tiles = N / 64;
  int sp = 1;
  while (sp < 16 && (long)tiles * sp * 2 <= 256 && K / (sp * 2) >= 512 && K % (sp * 2 * 256) == 0) sp *= 2;
  return sp;
}

// A launch: err < 0 for a shape / configuration the kernels do not take; else, unless mt == 0
// (no rows: nothing to launch), the form <mt, nt, epi, a_packed, waves> of `family` on a grid of
// (gx, slabs, experts) workgroups, each K slice kchunk deep.  slabs is the number of fp32 slabs an
// EPI_SLAB launch writes per expert.
struct SkinnyPlan {
  int err, family, mt, nt, waves, kchunk, slabs, gx;
};

// S <= 0: automatic split-K for EPI_SLAB (one slice for a grouped launch above kSkinnyMaxM rows).
// nt_tiles: 2 or 4 n-tiles per workgroup (the packed kernel; the row-major one picks 3 or 4).
// waves: 2 / 4 (row-major) or 8 (packed) forces a workgroup size, anything else leaves the choice.
constexpr SkinnyPlan skinny_plan(int M, int N, int K, int S, int epi, int nt_tiles, int a_packed, int waves,
                                 int experts, int w_rm) {
  if (M <= 0) return {};
  if (experts < 1) return {-5};
  if (epi < EPI_SLAB || epi > EPI_SWIGLU_PACKED) return {-1};
  const int mt = (M + 15) / 16;
  // 65..128 rows: grouped (expert) launches over row-major weights only - the EP all-to-all
  // decode's received rows (P x cap x top-k), so every local expert's weights stream ONCE per step
  // instead of once per 64-row chunk
  if (M > kSkinnyMaxM) {
    if (M > kSkinnyGroupedMaxM || !w_rm || experts < 2 || !a_packed || K % 64 != 0 || N % 64 != 0 ||
        (epi != EPI_SLAB && epi != EPI_SWIGLU_PACKED))
      return {-1};
    const int kc8 = skinny_kchunk(K, S <= 0 ? 1 : S, 64), slabs8 = (K + kc8 - 1) / kc8;
    if (epi != EPI_SLAB && slabs8 != 1) return {-3};
    return {0, SKINNY_RM, mt, 4, 2, kc8, slabs8, N / 64};
  }
  if (K % 32 != 0 || (nt_tiles != 2 && nt_tiles != 4) || N % (16 * nt_tiles) != 0) return {-1};
  if (S <= 0) S = epi == EPI_SLAB ? skinny_auto_splits(M, N, K) : 1;
  const int kc = skinny_kchunk(K, S, w_rm ? 64 : 32), slabs = (K + kc - 1) / kc;
  if (w_rm) {
    if (!a_packed || K % 64 != 0 || N % 64 != 0) return {-9};  // row-major W: packed A, 64-deep stages, NT = 4
    if (epi != EPI_SLAB && slabs != 1) return {-3};
    // split-K slab projections whose 64-column grid leaves CUs idle (qkv: 96 tiles x 2 slices =
    // 192 workgroups) use 48-column tiles when that fills the chip (128 x 2 = 256).
    if (epi == EPI_SLAB && N % 48 == 0 && (long)(N / 64) * slabs * experts < 224 &&
        (long)(N / 48) * slabs * experts <= 256)
      return {0, SKINNY_RM, mt, 3, 4, kc, slabs, N / 48};
    // 4 waves per workgroup unless the grid then needs more than one round of workgroups: each
    // wave's ring holds two 16-KiB stages at M = 64, so LDS caps residency (4 waves: 1 workgroup
    // per CU at MT 2-4); 2-wave workgroups keep e.g. gate_up's 448 tiles co-resident.
    constexpr int lds4[5] = {0, SkinnyRmGeom<1, 4, 0, 4>::LDS, SkinnyRmGeom<2, 4, 0, 4>::LDS,
                             SkinnyRmGeom<3, 4, 0, 4>::LDS, SkinnyRmGeom<4, 4, 0, 4>::LDS};
    // waves = 2 or 4 forces one.
    const bool one_round = (long)(N / 64) * slabs * experts <= 256L * (163840 / lds4[mt]);
    return {0, SKINNY_RM, mt, 4, waves == 2 || waves == 4 ? waves : one_round ? 4 : 2, kc, slabs, N / 64};
  }
  if (epi != EPI_SLAB && slabs != 1) return {-3};
  if ((epi == EPI_SWIGLU || epi == EPI_SWIGLU_PACKED) && nt_tiles != 4) return {-4};
  // 8-wave workgroups: twice the weight lines in flight per CU for the same K slice.  waves <= 0
  // (auto): 8 for the split-K slab projections (o 11.1 vs 11.8 us, down 24.3 vs 25.9 at M = 64),
  // 4 for the single-slice SwiGLU / bf16 epilogues (gate_up 47.5 vs 50.5 us).
  const int nwaves = waves == 8 || (waves <= 0 && epi == EPI_SLAB) ? 8 : 4;
  return {0, SKINNY_PACKED, mt, nt_tiles, nwaves, kc, slabs, N / (16 * nt_tiles)};
}

}  // namespace k8sllm
