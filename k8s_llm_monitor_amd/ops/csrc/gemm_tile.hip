// 256 x 256 MFMA GEMM for prefill-sized projections, dense or grouped
// over experts, with the SwiGLU activation fused into the epilogue.
//
//   Y[r][n] = sum_k X[r][k] * W[n][k]        (both operands K-contiguous: X [rows][K], W [N][K])
//
// Dense:   one weight, rows 0 .. M-1.
// Grouped: W [E][N][K]; expert e owns rows offsets[e] .. offsets[e+1]-1 of the expert-sorted X
//          (moe_align); each workgroup finds its (expert, m-tile) from the device offsets, so a
//          MoE layer needs no host synchronisation.
// EPI_SWIGLU: W is gate/up-interleaved per 128 rows ([64 gate | 64 up], ops.interleave_gate_up),
//          Y = silu(gate) * up [rows][N / 2] - the separate silu_mul pass over the [rows][N]
//          intermediate disappears.
// EPI_ROPE / EPI_RESID / RS: the qkv projection's rotary embedding, the o / down residual add +
//          next-RMSNorm operands, and the consumers' deferred 1/rms row scale (see TileEpi below).
//
// Structure: 4 waves (one per SIMD), each owning a 128 x 128 quarter of the tile as 64 accumulators
// of v_mfma_f32_16x16x32_bf16 (256 f32 per lane in AGPRs).  Per 32-deep k sub-step a wave reads 16
// ds_read_b128 for 64 MFMAs.
//  * K in 64-deep tiles with 128-B LDS rows, so every DMA row segment is one whole 128-B line.
//  * LDS = a ring of five 32 KiB half-slots (160 KiB, one __shared__ array); half-tile h (A_t = 2t,
//    B_t = 2t + 1) lives in slot h % 5, refilled by LDS-DMA (buffer_load_dwordx4 ... lds against
//    SGPR buffer descriptors of the tile's rows: lane offsets are per-lane constants, the k offset
//    goes in soffset).
//  * fragments of the next sub-step are read in between the current one's MFMAs into the second
//    register set: (t, 1) during (t, 0), (t + 1, 0) during (t, 1).
//  * 128-B LDS rows: logical 16-B chunk c of row r sits at physical chunk c ^ ((r >> 1) & 7)
//    (applied to the DMA source address; the LDS side is lane-linear), so each 16-lane group of a
//    fragment ds_read_b128 (rows 0-15 of a block) hits 16 distinct bank quads.
//  * XCD-aware tile order: workgroup ids are remapped so each XCD runs a contiguous range of
//    logical tiles, ordered in groups of 8 m-tiles (neighbours share A or B through that XCD's L2).
//
// Two refill schedules (SCH):
//  0: one barrier per k-tile, before (t, 1); A_{t+2} DMA'd during (t, 0), B_{t+2} during (t, 1),
//     pieces spread one per 8 MFMAs.
//  1: two barriers per k-tile: the mid-(t, 0) barrier (every wave holds tile t's k-half-1
//     fragments in registers) frees BOTH of tile t's half-slots, so B_{t+2} and A_{t+3} are DMA'd
//     from there on and every piece gets >= ~120 MFMAs to land.  2-6 % faster than SCH 0 on the
//     Llama-3-8B prefill shapes (profiles/r03/gemm_schedules.jsonl).  Its ring addressing is
//     scalar: the tile's five half-slot offsets advance in SGPRs (one conditional subtract) and each
//     sub-step forms one A and one B fragment base VGPR (block reads = base + immediate).  With
//     `(2t + i) % 5` written inline hipcc emitted ~25 mul-hi / per-read address instructions in
//     front of every k-tile's first MFMA; removing them made the kernel 4-5 % faster on every
//     shape (profiles/r03/gemm_ring_addressing.jsonl).
// Measured against hipBLASLt's own gfx950 256x256x64 kernel (profiles/r06/README.md): the same
// instruction mix per k-tile (128 MFMA, 32 ds_read_b128, 16 LDS-DMA pieces); ported its schedule
// (two whole-k-tile buffers, three barriers per k-tile, reads one per two MFMAs, its operand
// order) and four other row swizzles - all within +-1 % of this kernel, bit-identical, removed;
// the 5-7 % gap to it is per-tile and independent of the tile-wave count (1, 4, 16).
// Measured and removed (profiles/r03, r05): an 8-wave 128 x 64-per-wave kernel (0.375 reads per MFMA;
// the round-5 ping-pong form of it, bit-identical, 5-6 % slower), non-temporal residual-epilogue
// stores (-1.9 % on o in isolation, below what an end-to-end A/B resolves),
// a persistent form (spilled), register-staged refill (8-10 % slower: ds_write_b128 costs more
// than the DMA issue), the same tile on v_mfma_f32_32x32x16_bf16 (1-5 % slower), unswizzled rows
// (bank conflicts, 10-15 % slower), L1-bypass / nt cache policies and staggered per-wave issue
// (within 1 %).
//
// F8 (dense, schedule 1): W is the decode GEMMs' fp8 encoding - e4m3 codes fragment-packed
// [N/16][K/64][64][16] (ops.pack_skinny_f8) and one power-of-two scale per row - so a model needs no
// bf16 copy of a projection for prefill.  Block (n-tile j, k-tile) is one contiguous 1 KiB whose
// lane l holds its 8 codes of k sub-step 0, then of sub-step 1:
//  * a B half-tile is 16 KiB = 4 DMA pieces per wave (piece p = block 4p + wave of the tile), in
//    the first half of its 32 KiB half-slot.  The ring keeps its five 32 KiB half-slots (A and B
//    rotate through the same slots); the 16 KiB a B half-tile leaves free is not used.
//  * while sub-step s computes, a wave reads the 8 bytes of sub-step s+1's codes of each of its 8
//    blocks (ds_read_b64 at lane * 16 + 8 ks: lanes l and l + 16 share banks, so a read costs the
//    4 LDS cycles of the bf16 kernel's ds_read_b128 - the same LDS time per k-tile as there; one
//    16-B read for both sub-steps would halve it, but its 32 registers held across the k-tile
//    spilled) and converts them: v_cvt_scalef32_pk_bf16_fp8 with the scale of row
//    16 j + (lane & 15), two per MFMA shadow, 32 per sub-step.  code * 2^e is exact in bf16, so
//    the fragment registers hold exactly the bf16 weight: the MFMA sequence and every epilogue are
//    those of the bf16 kernel, and the result is bit-identical to it over the dequantised weight.
//
// F4 (dense, schedule 1): W is the decode GEMMs' mxfp4 encoding - e2m1 codes fragment-packed
// [N/16][K/128][64][16] and e8m0 block scales [N/16][K/128][16][4] (ops.pack_skinny_f4) - the one
// tensor decode streams.  A 1-KiB code block covers two k-tiles (lane l's dword s is its 8 codes of
// k-step 4 g + s), so the F8 form's structure is kept and only the indices change:
//  * a B half-tile is the same 4 code pieces per wave, of block (n-tile, kt >> 1): both k-tiles of a
//    pair fetch the same block (the second fetch is an L2 hit), plus ONE dword-wide piece per wave
//    for the scales - the 16 n-tiles' 64-B scale blocks of the pair are 1 KiB, kept at byte 16384 of
//    the half-slot (the half F8 leaves unused).  Every wave issues 5 pieces per B half-tile, so the
//    counted vmcnt waits are F8's plus one per B half-tile in flight.
//  * the codes of BOTH sub-steps of k-tile t + 1 are read once, while (t, 1) computes: one
//    ds_read_b64 per block at lane * 16 + 8 ((t + 1) & 1) (F8's bank pattern, 4 LDS cycles; half
//    F8's B-side reads), the second dword held for one sub-step.  Each sub-step reads the e8m0 byte
//    2 (kt & 1) + ks of row lane & 15 of each block (ds_read_u8; a 16-lane group reads 16
//    neighbouring dwords, the other groups the same ones) and MFMAs 16-18 shift the 8 bytes into
//    fp32 exponents (<< 23), so the 16 conversion units stay two instructions each, in F8's MFMA
//    shadows: four v_cvt_scalef32_pk_bf16_fp4 per fragment with the scale applied inside
//    (gemm_decode.hip dec_f4x8).  code * 2^e is exact in bf16: bit-identical to the bf16 kernel
//    over the dequantised weight.  (The first form - a ds_read_b32 of the code dword per sub-step,
//    a 4-way bank conflict at the 16-B lane stride, and the scale dword with v_bfe + shift inside
//    every other conversion unit, four dependent VALU in one MFMA shadow - was 5.5-8.5 % slower than
//    bf16 on the Llama-3-8B projections; this one is 1.4-3.0 %: profiles/r16/README.md.)
#include <type_traits>

#include "common.h"
#include "tile_epi.h"

namespace k8sllm {

namespace {
typedef __attribute__((address_space(3))) void lds_void_t;

template <int N>
__device__ __forceinline__ void vm_wait_n() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void lgkm_wait0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
}  // namespace

// PERSIST (dense bf16 W, schedule 1; the instantiations of kTilePersist): the grid is min(tiles,
// CUs) and a workgroup walks the tiles bid, bid + grid, ... (each through the same XCD remap and
// m-tile grouping, so with a grid that is a multiple of 8 it stays inside its XCD's range), with a
// seam in place of workgroup exit + start-up + an unoverlapped ring fill:
//  * once every wave is done with the ring (the barrier in front of the epilogue) the NEXT tile's
//    A_0 and B_0 are DMA'd into half-slots 0 and 1;
//  * the epilogue stages through half-slots 2 - 4 only, in two passes of 64 rows per wave (4 waves x
//    64 rows x 272 B = 68 KiB, + the row scales' 1 KiB behind them);
//  * after the last staging read (a barrier: a wave's pieces land in every wave's staging rows)
//    A_1, B_1 and A_2 follow into half-slots 2 - 4, and the epilogue's global stores drain under
//    them and under the next tile's first k-tile.
// Waits at the seam.  vmcnt counts loads, LDS-DMA pieces and stores alike and retires them in issue
// order, so the one counted wait is the tile's first, whatever the epilogue issued: a wave's
// outstanding operations are then, oldest first, [A_0 B_0: 16 pieces] [the epilogue's loads and
// stores: any number] [A_1 B_1 A_2: 24 pieces], and vmcnt(24) retires everything but the last 24 -
// tile 0 has landed (and the stores are done) exactly as after the first tile's prologue, where the
// 40 pieces are issued back to back.  Every later wait of the k loop counts ring pieces only, as in
// the one-tile form.  Nothing else may wait on vmcnt while pieces fly, so at the seam the row-scale
// exchange uses a raw s_barrier (a __syncthreads() would drain them) and the row-scale partials are
// loaded during the tile's LAST k-tile (like RESID's residual rows) and summed before the seam's
// DMAs are issued, not in the prologue.  Each output element sees the same MFMA sequence and the
// same epilogue arithmetic: bit-identical to the one-tile form.
template <int EPI, bool GROUPED, int SCH, bool RS = false, bool F8 = false, bool F4 = false, bool PERSIST = false>
__global__ __launch_bounds__(256, 1) void gemm_w4_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W,
                                                         bf16_t* __restrict__ Y, const int* __restrict__ offsets,
                                                         int E, int M, int N, int K, long w_es, int n_mt, int n_nt,
                                                         TileEpi ep, int wpk, const float* __restrict__ wscale) {
  static_assert(!F8 || (SCH == 1 && !GROUPED), "the fp8-W form is dense, schedule 1");
  static_assert(!F4 || (SCH == 1 && !GROUPED && !F8), "the mxfp4-W form is dense, schedule 1");
  static_assert(!PERSIST || (SCH == 1 && !GROUPED && !F8 && !F4), "the persistent form is dense, bf16 W, schedule 1");
  constexpr bool FQ = F8 || F4;  // W arrives as codes: 4 code pieces per B half-tile, fragments converted in registers
  constexpr int HS = 32768;  // one half-slot: 256 rows x 128 B
  __shared__ __attribute__((aligned(16))) char smem[5 * HS];
  int lane = threadIdx.x & 63;
  int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int wm = wave >> 1, wn = wave & 1;
  int tid = threadIdx.x;
  // PERSIST: what is made from the lane and wave ids (fragment and staging addresses, DMA lane
  // offsets, LDS piece addresses) is made again per tile and at the seam, from ids the compiler
  // cannot see through.  Left loop-invariant they are hoisted out of the tile loop and live across
  // the k loop AND the epilogue: the scalars overflow the SGPR file into VGPR lanes, the lane
  // constants spill, and a spill's reload waits vmcnt(0) - for the pieces in flight at the seam
  auto fresh_ids = [&]() {
    if constexpr (PERSIST) {
      int w = wave;
      asm volatile("" : "+v"(lane), "+v"(w));
      wave = __builtin_amdgcn_readfirstlane(w);
      tid = wave * 64 + lane;
      wm = wave >> 1;
      wn = wave & 1;
    }
  };

  // ---- logical tile: bijective XCD remap, then groups of 8 m-tiles ----
  const int nwg = n_mt * n_nt;
  const int bid = blockIdx.x, xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  constexpr int GM = 8;
  const int grp = lid / (GM * n_nt), first_m = grp * GM;
  const int gsz = min(n_mt - first_m, GM);
  const int in_g = lid - grp * GM * n_nt;
  const int mt = first_m + in_g % gsz, nt = in_g / gsz;

  int row0, mrows;
  const bf16_t* Wt = W;
  if constexpr (GROUPED) {
    int e = -1, acc_t = 0;
    row0 = 0;
    mrows = 0;
    for (int x = 0; x < E; ++x) {
      const int o0 = offsets[x], o1 = offsets[x + 1];
      const int tiles = (o1 - o0 + 255) >> 8;
      if (e < 0 && mt < acc_t + tiles) {
        e = x;
        row0 = o0 + (mt - acc_t) * 256;
        mrows = min(256, o1 - row0);
      }
      acc_t += tiles;
    }
    if (e < 0) return;  // uniform: past the last expert's tiles
    Wt = W + (long)e * w_es;
  } else {
    row0 = mt * 256;
    mrows = min(256, M - row0);
  }
  int n0 = nt * 256;
  int nrows = min(256, N - n0);

  // ---- DMA of one half-tile (256 rows x 128 B = 32 pieces of 1 KiB): piece p (0..7) of this
  // wave covers rows (p * 4 + wave) * 8 .. + 7; lane -> row + (lane >> 3), physical chunk lane & 7 ----
  uint32_t soff[2][8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int rl = (p * 4 + wave) * 8 + (lane >> 3);
    const int cl = (lane & 7) ^ ((rl >> 1) & 7);
    soff[0][p] = (uint32_t)(((long)min(rl, mrows - 1) * K + cl * 8) * 2);  // rows past the end: clamped, never stored
    soff[1][p] = (uint32_t)(((long)min(rl, nrows - 1) * K + cl * 8) * 2);
    if constexpr (FQ) {  // e4m3 codes [N/16][K/64][64][16]: piece p < 4 = the 1-KiB block (n-tile 4 p + wave, k-tile;
      // F4, e2m1 codes [N/16][K/128][64][16]: k-tile pair):
      // the block's offset is wave-uniform (sB below, in the soffset); the lane part is lane * 16
      soff[1][p] = (uint32_t)(lane * 16);
    } else if (wpk) {  // W fragment-packed [N/16][K/32][64][8]: piece = one contiguous 1-KiB block (n-tile, k-step)
      const int blk = p * 4 + wave, j = min(blk >> 1, (nrows >> 4) - 1);
      soff[1][p] = (uint32_t)(((long)j * (K >> 5) + (blk & 1)) * 1024 + lane * 16);
    }
  }
  // F8: byte offset of piece p's block row (n-tile 4 p + wave; the ragged last n-tile clamps, those
  // rows are never stored) in this tile's W range - scalar
  uint32_t sB[4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
    sB[p] = F4   ? (uint32_t)(min(p * 4 + wave, (nrows >> 4) - 1) * (K >> 7)) * 1024u
            : F8 ? (uint32_t)(min(p * 4 + wave, (nrows >> 4) - 1) * (K >> 6)) * 1024u
                 : 0u;
  const int kstrB = F8 ? 1024 : wpk ? 2048 : 128;  // bytes of W per k-tile step, in the piece's soffset
  constexpr int WB = F8 ? 1 : 2;                    // bytes per W element (F4: half a byte, below)
  // F4: the e8m0 block scales [N/16][K/128][16][4] ride as a fifth, dword-wide piece: wave w brings
  // the 64-B scale blocks of n-tiles 4 w .. 4 w + 3 of the k-tile pair (lane l: dword l & 15 of
  // n-tile 4 w + (l >> 4), clamped like the codes) to bytes 16384 + 256 w .. of the B half-slot -
  // there the 16 n-tiles' blocks lie in order, 64 B each
  [[maybe_unused]] uint32_t soffS = 0u;
  if constexpr (F4) soffS = (uint32_t)(min(wave * 4 + (lane >> 4), (nrows >> 4) - 1) * (K >> 7) * 64 + (lane & 15) * 4);
  // buffer descriptors over this tile's X rows / W rows, built from wave-uniform values only so
  // hipcc keeps them in SGPRs (no waterfall loops, cdna_hip_programming.md T20)
  auto rsrc = [](const void* base, long bytes) {
    const uint64_t a = reinterpret_cast<uint64_t>(base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    const int nb = __builtin_amdgcn_readfirstlane((int)bytes);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, nb, 0x00020000);
  };
  __amdgpu_buffer_rsrc_t xr = rsrc(reinterpret_cast<const char*>(X) + (long)row0 * K * 2, (long)mrows * K * 2);
  // F4: half a byte per element; sr: the tile's scale blocks, (nrows / 16)(K / 128) of 64 B
  const auto wdesc = [&] {
    if constexpr (F4) return rsrc(reinterpret_cast<const char*>(Wt) + (long)n0 * K / 2, (long)nrows * K / 2);
    else return rsrc(reinterpret_cast<const char*>(Wt) + (long)n0 * K * WB, (long)nrows * K * WB);
  };
  __amdgpu_buffer_rsrc_t wr = wdesc();
  const auto sdesc = [&] {
    if constexpr (F4)
      return rsrc(reinterpret_cast<const char*>(wscale) + (long)(n0 >> 4) * (K >> 7) * 64, (long)(nrows >> 4) * (K >> 7) * 64);
    else return wr;
  };
  [[maybe_unused]] __amdgpu_buffer_rsrc_t sr = sdesc();
  const int nk = K >> 6;
  // PERSIST, at the seam: the same again for tile vb of this workgroup's walk (dense, bf16 W) - its
  // coordinates (tile_of) and what its pieces need (dma_setup: the lane offsets and the two
  // descriptors above, recomputed there and not carried over the tile loop in registers)
  struct Tile {
    int row0, mrows, n0, nrows;
  };
  [[maybe_unused]] auto tile_of = [&](int vb) -> Tile {
    const int vx = vb & 7;
    const int vl = (vx < r8 ? vx * (q8 + 1) : r8 * (q8 + 1) + (vx - r8) * q8) + (vb >> 3);
    const int vg = vl / (GM * n_nt), vf = vg * GM;
    const int vs = min(n_mt - vf, GM);
    const int vi = vl - vg * GM * n_nt;
    const int vm = vf + vi % vs, vn = vi / vs;
    return Tile{vm * 256, min(256, M - vm * 256), vn * 256, min(256, N - vn * 256)};
  };
  [[maybe_unused]] auto dma_setup = [&](const Tile& t) {
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int rl = (p * 4 + wave) * 8 + (lane >> 3);
      const int cl = (lane & 7) ^ ((rl >> 1) & 7);
      soff[0][p] = (uint32_t)(((long)min(rl, t.mrows - 1) * K + cl * 8) * 2);
      soff[1][p] = (uint32_t)(((long)min(rl, t.nrows - 1) * K + cl * 8) * 2);
      if (wpk) {
        const int blk = p * 4 + wave, j = min(blk >> 1, (t.nrows >> 4) - 1);
        soff[1][p] = (uint32_t)(((long)j * (K >> 5) + (blk & 1)) * 1024 + lane * 16);
      }
    }
    xr = rsrc(reinterpret_cast<const char*>(X) + (long)t.row0 * K * 2, (long)t.mrows * K * 2);
    wr = rsrc(reinterpret_cast<const char*>(W) + (long)t.n0 * K * 2, (long)t.nrows * K * 2);
  };

  // piece p of half-tile (operand o, k-tile kt) into half-slot `slot`; k-tiles past the end re-read
  // the last one (identical bytes into a slot no live fragment read uses), so every sub-step
  // issues the same count and the vmcnt arithmetic never changes
  auto piece = [&](int o, int p, int kt, int slot) {
    char* dst = smem + slot * HS + (p * 4 + wave) * 1024;
    if constexpr (F4) {
      if (o && p == 4) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(sr, (lds_void_t*)(smem + slot * HS + 16384 + wave * 256), 4, soffS,
                                                 (min(kt, nk - 1) >> 1) * 64, 0, 0);
        return;
      } else if (o) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_void_t*)dst, 16, soff[1][p],
                                                 (min(kt, nk - 1) >> 1) * 1024 + sB[p], 0, 0);
        return;
      }
    }
    if (o)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_void_t*)dst, 16, soff[1][p], min(kt, nk - 1) * kstrB + sB[p & 3], 0, 0);
    else
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_void_t*)dst, 16, soff[0][p], min(kt, nk - 1) * 128, 0, 0);
  };
  auto issue_half = [&](int o, int kt) {
#pragma unroll
    for (int p = 0; p < (F4 && o ? 5 : F8 && o ? 4 : 8); ++p) piece(o, p, kt, (2 * kt + o) % 5);
  };

  // fragment read: lane row lane & 15 of a 16-row block, 16-B chunk 4 ks + (lane >> 4)
  int rd[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) rd[ks] = (lane & 15) * 128 + (((4 * ks + (lane >> 4)) ^ ((lane >> 1) & 7)) << 4);
  // packed W: the LDS image is the blocks verbatim, block (n-tile, k-step) at (2 n-tile + k-step) KiB:
  // every fragment read is lane-linear (conflict-free without a swizzle)
  int rdB[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) rdB[ks] = wpk ? ks * 1024 + lane * 16 : rd[ks];
  auto frag = [&](int slot, int ks, int o, int blk) -> bf16x8 {
    return *reinterpret_cast<const bf16x8*>(smem + slot * HS + ((o ? wn : wm) * 8 + blk) * 2048 + (o ? rdB[ks] : rd[ks]));
  };

  // ---- one tile; PERSIST: every tile vb = bid, bid + grid, ... of this workgroup, row0 .. nrows the
  // current one's (its ring pieces A_0 B_0 A_1 B_1 A_2 issued by the prologue below for the first
  // tile, at the seam for the others), nx the next one's from the seam on ----
  [[maybe_unused]] bool first = true, more = false;
  [[maybe_unused]] int vb = bid;
  [[maybe_unused]] Tile nx{};
  do {
    fresh_ids();
    if constexpr (PERSIST) {  // the fragment read offsets, per tile
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        rd[ks] = (lane & 15) * 128 + (((4 * ks + (lane >> 4)) ^ ((lane >> 1) & 7)) << 4);
        rdB[ks] = wpk ? ks * 1024 + lane * 16 : rd[ks];
      }
    }
    float rs_inv = 1.f;  // RS: 1 / rms of this thread's row (threadIdx.x of the tile)
    f32x4 acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    // F8: the B fragments are built a dword (two bf16) at a time, so they are held as dwords
    using fragb_t = std::conditional_t<FQ, u32x4, bf16x8>;
    bf16x8 fa0[8], fa1[8];
    fragb_t fb0[8], fb1[8];
    // F8: the next sub-step's 8 codes of each of the wave's 8 blocks as read from LDS, and the scale
    // of this lane's row of each block
    u32x2 raw[FQ ? 8 : 1];
    float wsc[F8 ? 8 : 1];
    // F4: raw[b] holds BOTH sub-steps' code dwords of a k-tile (one 8-byte read per block and k-tile,
    // made while the previous tile's second sub-step computes); sraw[b] is the e8m0 byte of this
    // lane's row of block b for the next sub-step as read from LDS, then (in place) << 23, its fp32
    uint32_t sraw[F4 ? 8 : 1];
    auto cvt4q = [](u32x4& d, uint32_t c, float sc, int h) {  // bytes 2 h, 2 h + 1 of c -> dwords 2 h, 2 h + 1 (dec_f4x8)
      typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
      if (h == 0) {
        d[0] = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 0));
        d[1] = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 1));
      } else {
        d[2] = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 2));
        d[3] = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 3));
      }
    };
    // 4 codes (one dword) x the row scale -> dwords 2 h, 2 h + 1 of a fragment; exact (common.h kv_f8_deq8)
    auto cvt4 = [](u32x4& d, uint32_t c, float sc, int h) {
      typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
      d[2 * h] = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c, sc, false));
      d[2 * h + 1] = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c, sc, true));
    };
    // RESID: this lane's first 16 residual chunks (rows rr + 4b of the wave's 128, 16 B at column
    // chunk cc), issued during the last k-tile's second half so they land behind its MFMAs
    u32x4 resq[EPI == TILE_EPI_RESID ? 16 : 1];

    if constexpr (SCH == 1) {
      // Ring addressing: the half-slot byte offsets of the current tile live in SGPRs and rotate
      // by one conditional subtract per tile, and each sub-step forms ONE A and ONE B fragment base
      // VGPR (every block read is that base + an immediate).
      const uint32_t fbA0 = (uint32_t)(rd[0] + wm * 16384), fbA1 = (uint32_t)(rd[1] + wm * 16384);
      const uint32_t fbB0 = (uint32_t)(rdB[0] + wn * 16384), fbB1 = (uint32_t)(rdB[1] + wn * 16384);
      auto rd16 = [&](uint32_t base, int blk) -> bf16x8 {
        return *reinterpret_cast<const bf16x8*>(smem + base + blk * 2048);
      };
      const uint32_t fbR = (uint32_t)(lane * 16 + wn * 8192);  // F8: block blk of the wave's 8, 1 KiB each
      auto rdraw = [&](uint32_t base, int blk) -> u32x2 {
        return *reinterpret_cast<const u32x2*>(smem + base + blk * 1024);
      };
      // F4: the scale dword of this lane's row (lane & 15) of block 0 of the wave's 8, behind the codes;
      // block blk is 64 blk further, the sub-step's byte is added in sub
      [[maybe_unused]] uint32_t fbS = 0u;
      if constexpr (F4) fbS = (uint32_t)(16384 + wn * 512 + (lane & 15) * 4);
      auto rd8 = [&](uint32_t base, int off) -> uint32_t { return *reinterpret_cast<const uint8_t*>(smem + base + off); };
      auto pc = [&](int o, int p, int kt, uint32_t slot_bytes) {
        char* dst = smem + slot_bytes + (p * 4 + wave) * 1024;
        if constexpr (F4) {
          if (o) {
            if (p == 4)
              __builtin_amdgcn_raw_ptr_buffer_load_lds(sr, (lds_void_t*)(smem + slot_bytes + 16384 + wave * 256), 4, soffS,
                                                       (min(kt, nk - 1) >> 1) * 64, 0, 0);
            else
              __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_void_t*)dst, 16, soff[1][p],
                                                       (min(kt, nk - 1) >> 1) * 1024 + sB[p], 0, 0);
            return;
          }
        }
        __builtin_amdgcn_raw_ptr_buffer_load_lds(o ? wr : xr, (lds_void_t*)dst, 16, soff[o][p],
                                                 min(kt, nk - 1) * (o ? kstrB : 128) + (o ? sB[p & 3] : 0u), 0, 0);
      };
      // PM (the ring tail, peeled): 0 = B_{t+2} and A_{t+3} refills; 1 = B_{t+2} only (A_{t+3} is
      // past the end); 2 = no refill; 3 = no refill and, in (t, 1), no reads of tile t+1 (there is
      // none).  The tail issues no dummy pieces (a re-read of the last k-tile kept the counts fixed:
      // 40 of every tile's 1064 pieces per wave, ~4 % of the DMA issue at K = 4096).
      auto sub = [&](auto ph, auto pm, bf16x8 (&ca)[8], fragb_t (&cb)[8], bf16x8 (&na)[8], fragb_t (&nb)[8],
                     uint32_t sa, uint32_t sb, uint32_t da, uint32_t db, int t) {
        constexpr int PH = decltype(ph)::value, PM = decltype(pm)::value;
        constexpr bool READS = !(PH == 1 && PM == 3);
        // sa / sb: half-slot bytes of the fragments read here; da / db: B_{t+2}'s / A_{t+3}'s targets
        const uint32_t ba = sa + (PH == 0 ? fbA1 : fbA0), bb = sb + (PH == 0 ? fbB1 : fbB0);
        // F4: the sub-step read here is k-step 2 (t + PH) + (1 - PH): scale byte 2 ((t + PH) & 1) + (1 - PH)
        // of its k-tile pair (bsq: its address in block 0); the codes of both sub-steps of k-tile t + 1 are read in
        // (t, 1), 8 bytes at bcq: dwords 2 ((t + 1) & 1), + 1 of the pair's block
        [[maybe_unused]] uint32_t bcq = 0u, bsq = 0u;
        if constexpr (F4) {
          bcq = sb + fbR + 8 * ((t + 1) & 1);
          bsq = sb + fbS + 2 * ((t + PH) & 1) + (1 - PH);
        }
        // F4: B_{t+2} is 5 pieces (4 of codes, 1 of scales), MFMAs 22, 31, .., 58 of (t, 0)
        constexpr int NPB = F4 ? 5 : 4, PST = F4 ? 9 : 12;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int n = g * 8 + j;
            acc[g][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cb[j]), ca[g], acc[g][j], 0, 0, 0);
            if constexpr (FQ) {
              // One instruction group per MFMA shadow, as below.  B_{t+2} is 4 pieces (MFMAs 22, 34,
              // 46, 58 of (t, 0)) and A_{t+3}'s 8 ride MFMAs 19, 24, .., 54 of (t, 1).  MFMAs 0-7 read
              // the next sub-step's codes of the 8 blocks, 8-15 its A fragments; behind them the 16
              // conversion units (unit u: fragment u >> 1, code dword u & 1 -> fragment dwords
              // 2 (u & 1), + 1: two v_cvt) take the non-piece MFMAs from 20 on - (t, 0): 20 .. 37
              // without 22, 34, after the barrier's wait for the reads; (t, 1): 20 .. 38 without 24,
              // 29, 34.  nb was the previous sub-step's cb: all of its MFMAs have issued (in order)
              // long before the first unit, and an MFMA reads its A / B operands when it issues.
              const int cu = n < 20 ? -1
                             : PH == 0 ? (n <= 37 && n != 22 && n != 22 + PST ? (n - 20) - (n > 22) - (n > 22 + PST) : -1)
                                       : (n < 39 && (n - 19) % 5 != 0 ? (n - 20) - (n - 19) / 5 : -1);
              if (n < 8) {
                if constexpr (READS && F4) {
                  if constexpr (PH == 1) raw[n] = rdraw(bcq, n);
                  sraw[n] = rd8(bsq, n * 64);
                } else if constexpr (READS) {
                  raw[n] = rdraw(sb + fbR + (PH == 0 ? 8 : 0), n);
                }
              } else if (n < 16) {
                if constexpr (READS) na[n - 8] = rd16(ba, n - 8);
              } else if (F4 && n < 19) {  // F4: MFMAs 16-18 turn the 8 scale bytes (read 9+ MFMAs ago) into fp32s
                if constexpr (READS && F4) {
#pragma unroll
                  for (int i = 3 * (n - 16); i < (n == 18 ? 8 : 3 * (n - 15)); ++i) sraw[i] <<= 23;
                }
              } else if (cu >= 0) {
                if constexpr (READS && F4) {
                  cvt4q(nb[cu >> 1], raw[cu >> 1][PH == 0 ? 1 : 0], __uint_as_float(sraw[cu >> 1]), cu & 1);
                } else if constexpr (READS) {
                  cvt4(nb[cu >> 1], raw[cu >> 1][cu & 1], wsc[cu >> 1], cu & 1);
                }
              } else if (PH == 0 && PM <= 1 && n == 19) {  // frees tile t's half-slots for the refills
                lgkm_wait0();
                __builtin_amdgcn_s_barrier();
              } else if (PH == 0 && PM <= 1 && n >= 22 && (n - 22) % PST == 0 && (n - 22) / PST < NPB) {
                pc(1, (n - 22) / PST, t + 2, da);
              } else if (PH == 1 && PM == 0 && n >= 19 && (n - 19) % 5 == 0 && (n - 19) / 5 < 8) {
                pc(0, (n - 19) / 5, t + 3, db);
              }
            } else if (n < 8) {
              if constexpr (READS) nb[n] = rd16(bb, n);
            } else if (n < 16) {
              if constexpr (READS) na[n - 8] = rd16(ba, n - 8);
            } else if (PH == 0 && PM <= 1 && n == 19) {  // frees tile t's half-slots for the refills
              lgkm_wait0();
              __builtin_amdgcn_s_barrier();
            } else if (PH == 0 && PM <= 1 && n >= 22 && (n - 22) % 6 == 0 && (n - 22) / 6 < 7) {
              pc(1, (n - 22) / 6, t + 2, da);
            } else if (PH == 1 && PM <= 1 && n >= 19 && (n - 19) % 5 == 0 && (n - 19) / 5 < 9) {
              const int i = 7 + (n - 19) / 5;
              if (i < 8)
                pc(1, i, t + 2, da);
              else if (PM == 0)
                pc(0, i - 8, t + 3, db);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      };
      using P0 = std::integral_constant<int, 0>;
      using P1 = std::integral_constant<int, 1>;
      using P2 = std::integral_constant<int, 2>;
      using P3 = std::integral_constant<int, 3>;
      // RS: this thread's row partials (row row0 + tid, clamped), loaded ahead of the prologue DMAs
      // so their wait is the prologue's own (a fixed 16 loads: up to 64 partials, extra ones masked)
      // (PERSIST: loaded during the tile's last k-tile and summed behind the k loop - nothing but ring
      // pieces may be waited for between the seam's DMAs and here)
      f32x4 rsq[RS ? 16 : 1];
      if constexpr (RS && !PERSIST) {
        const float* rp = ep.rs_part + (long)(row0 + min((int)threadIdx.x, mrows - 1)) * ep.rs_np;
#pragma unroll
        for (int j = 0; j < 16; ++j) rsq[j] = *reinterpret_cast<const f32x4*>(rp + min(4 * j, ep.rs_np - 4));
      }
      if constexpr (F8) {  // scale of row 16 j + (lane & 15) of the wave's 8 blocks (past N: clamped, never stored)
#pragma unroll
        for (int g = 0; g < 8; ++g) wsc[g] = wscale[min(n0 + (wn * 8 + g) * 16 + (lane & 15), N - 1)];
      }
      if (!PERSIST || first) {
        issue_half(0, 0);
        issue_half(1, 0);
        issue_half(0, 1);
        issue_half(1, 1);
        issue_half(0, 2);
      }
      // tile 0 landed: younger are A_1 B_1 A_2 = 8 + 8 + 8 pieces; F8 (B = 4 pieces): 8 + 4 + 8; F4 (5): 8 + 5 + 8
      // (PERSIST, after a seam: the same last 24, with the epilogue's stores among the older ones)
      if constexpr (F4) vm_wait_n<21>(); else if constexpr (F8) vm_wait_n<20>(); else vm_wait_n<24>();
      __builtin_amdgcn_s_barrier();
      if constexpr (RS && !PERSIST) {
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (4 * j < ep.rs_np) sum += (rsq[j][0] + rsq[j][1]) + (rsq[j][2] + rsq[j][3]);
        rs_inv = rsqrtf(sum / (float)K + ep.rs_eps);
        // F8: pin the sum here (the compiler otherwise sinks it behind the k loop and keeps the 64
        // partial-sum registers alive across it, which with the raw codes no longer fit)
        if constexpr (FQ) asm volatile("" : "+v"(rs_inv));
      }
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        fa0[g] = frag(0, 0, 0, g);
        if constexpr (F4) {  // k-tile 0: dwords 0, 1 of the pair's block; k-step 0: dword 0, scale byte 0
          raw[g] = rdraw(HS + fbR, g);
          sraw[g] = rd8(HS + fbS, g * 64) << 23;
          cvt4q(fb0[g], raw[g][0], __uint_as_float(sraw[g]), 0);
          cvt4q(fb0[g], raw[g][0], __uint_as_float(sraw[g]), 1);
        } else if constexpr (F8) {
          raw[g] = rdraw(HS + fbR, g);
          cvt4(fb0[g], raw[g][0], wsc[g], 0);
          cvt4(fb0[g], raw[g][1], wsc[g], 1);
        } else {
          fb0[g] = frag(1, 0, 1, g);
        }
      }
      // half-slot bytes of tile t: S0 = (2t % 5) HS (A_t), S1 = ((2t + 1) % 5) HS (B_t), S2 / S3 =
      // tile t+1's.  Tile t+1: S0' = S2, S1' = S3, S2' = ((2t + 4) % 5) HS, S3' = S0.
      uint32_t S0 = 0, S1 = HS, S2 = 2 * HS, S3 = 3 * HS;
      auto rotate = [&]() {
        const uint32_t s4 = S0 == 0 ? 4 * HS : S0 - HS, s0 = S0;
        S0 = S2;
        S1 = S3;
        S2 = s4;
        S3 = s0;
      };
      // vmcnt at the mid-tile wait: B_{t+1} must have landed; younger are A_{t+2} (8) + B_{t+2}'s
      // first 7 pieces (15) in the steady state and at t = nk - 3, nothing from t = nk - 2 on.
      // F8: A_{t+2} (8) + all 4 pieces of B_{t+2}, issued in (t, 0) (12); F4: all 5 (13)
      constexpr int MIDW = F4 ? 13 : F8 ? 12 : 15;
      for (int t = 0; t < nk - 3; ++t) {
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the previous sub-step's reads, explicitly
        sub(P0{}, P0{}, fa0, fb0, fa1, fb1, S0, S1, S0, S1, t);
        vm_wait_n<MIDW>();
        __builtin_amdgcn_s_barrier();
        sub(P1{}, P0{}, fa1, fb1, fa0, fb0, S2, S3, S0, S1, t);
        rotate();
      }
      {  // t = nk - 3 (host: nk >= 3): B_{nk-1} is the last refill
        const int t = nk - 3;
        __builtin_amdgcn_s_waitcnt(0xc07f);
        sub(P0{}, P1{}, fa0, fb0, fa1, fb1, S0, S1, S0, S1, t);
        vm_wait_n<MIDW>();
        __builtin_amdgcn_s_barrier();
        sub(P1{}, P1{}, fa1, fb1, fa0, fb0, S2, S3, S0, S1, t);
        rotate();
      }
      {  // t = nk - 2: every piece issued so far must land (B_{nk-1} is read in (t, 1))
        const int t = nk - 2;
        __builtin_amdgcn_s_waitcnt(0xc07f);
        sub(P0{}, P2{}, fa0, fb0, fa1, fb1, S0, S1, S0, S1, t);
        vm_wait_n<0>();
        __builtin_amdgcn_s_barrier();
        sub(P1{}, P2{}, fa1, fb1, fa0, fb0, S2, S3, S0, S1, t);
        rotate();
      }
      {  // t = nk - 1: the last k-tile; (t, 1) reads nothing - RESID issues its residual loads here
        const int t = nk - 1;
        __builtin_amdgcn_s_waitcnt(0xc07f);
        sub(P0{}, P3{}, fa0, fb0, fa1, fb1, S0, S1, S0, S1, t);
        if constexpr (EPI == TILE_EPI_RESID) {
          const __amdgpu_buffer_rsrc_t rres = rsrc(ep.resid + (long)row0 * N, (long)mrows * N * 2);
          const uint32_t ro = (uint32_t)(((wm * 128 + (lane >> 4)) * N + n0 + wn * 128 + (lane & 15) * 8) * 2);
#pragma unroll
          for (int b = 0; b < 16; ++b)
            resq[b] = __builtin_amdgcn_raw_buffer_load_b128(rres, ro + (uint32_t)(4 * b * N * 2), 0, 0);
        }
        // PERSIST: the prologue's loads, here - they land behind the last 64 MFMAs (np, kk: the
        // tile-invariant offsets, masks and 1 / K made here, not kept in registers over the tile loop)
        [[maybe_unused]] int np = ep.rs_np, kk = K;
        if constexpr (RS && PERSIST) {
          asm volatile("" : "+s"(np), "+s"(kk));
          const float* rp = ep.rs_part + (long)(row0 + min(tid, mrows - 1)) * np;
#pragma unroll
          for (int j = 0; j < 16; ++j) rsq[j] = *reinterpret_cast<const f32x4*>(rp + min(4 * j, np - 4));
        }
        sub(P1{}, P3{}, fa1, fb1, fa0, fb0, S2, S3, S0, S1, t);
        if constexpr (RS && PERSIST) {  // the prologue's sum, pinned in front of the seam
          float sum = 0.f;
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (4 * j < np) sum += (rsq[j][0] + rsq[j][1]) + (rsq[j][2] + rsq[j][3]);
          rs_inv = rsqrtf(sum / (float)kk + ep.rs_eps);
          asm volatile("" : "+v"(rs_inv));
        }
      }
    } else {
      // One 32-deep sub-step: 64 MFMAs from (ca, cb), each carrying at most one other instruction in
      // its shadow.  The 8 DMA pieces of the sub-step ride MFMAs 4, 12, ..., 60 - evenly spread: an
      // LDS-DMA instruction holds its wave's issue for tens of cycles (MI355X_MICROARCH.md, LDS-DMA
      // piece issue cost), and bunched pieces starve the matrix pipe (all 16 pieces of a k-tile in
      // one sub-step: 8-13 % slower).  The 16 fragment reads of the next sub-step ride the other
      // MFMAs from the first on (W blocks first), done by MFMA 17.
      auto sub = [&](bf16x8 (&ca)[8], bf16x8 (&cb)[8], bf16x8 (&na)[8], bf16x8 (&nb)[8], int sa, int sb, int nks,
                     int o, int kt, int ds) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int n = g * 8 + j;
            acc[g][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cb[j], ca[g], acc[g][j], 0, 0, 0);
            const int q = n - (n > 4) - (n > 12);  // read index: skips the DMA slots 4 and 12
            if (j == 4) {
              piece(o, g, kt, ds);
            } else if (q < 8) {
              nb[q] = frag(sb, nks, 1, q);
            } else if (q < 16) {
              na[q - 8] = frag(sa, nks, 0, q - 8);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      };
      // prologue: A_0 B_0 A_1 B_1 in flight; tile 0 landed -> read its first k-half
      issue_half(0, 0);
      issue_half(1, 0);
      issue_half(0, 1);
      issue_half(1, 1);
      vm_wait_n<16>();
      __builtin_amdgcn_s_barrier();
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        fa0[g] = frag(0, 0, 0, g);
        fb0[g] = frag(1, 0, 1, g);
      }
      for (int t = 0; t < nk; ++t) {
        const int sa = (2 * t) % 5, sb = (2 * t + 1) % 5;        // tile t's half-slots
        const int sa1 = (2 * t + 2) % 5, sb1 = (2 * t + 3) % 5;  // tile t+1's
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): see SCH 1
        // (t, 0): MFMAs on k-half 0; read k-half 1 of tile t; DMA A_{t+2}
        sub(fa0, fb0, fa1, fb1, sa, sb, 1, 0, t + 2, (2 * t + 4) % 5);
        lgkm_wait0();
        vm_wait_n<8>();  // B_{t+1} landed (only A_{t+2} younger)
        __builtin_amdgcn_s_barrier();
        // (t, 1): MFMAs on k-half 1; read k-half 0 of tile t+1 (garbage past the end, never used); DMA B_{t+2}
        sub(fa1, fb1, fa0, fb0, sa1, sb1, 0, 1, t + 2, (2 * t + 5) % 5);
      }
      vm_wait_n<0>();
    }

    // ---- epilogue: acc[i][j][r] = Y[m][n], m = wm*128 + i*16 + (lane & 15),
    // n = wn*128 + j*16 + 4 (lane >> 4) + r.  Staged through LDS (the ring is idle now): each wave
    // writes its quarter as bf16 rows (8-B ds_write per 4 columns), then reads back whole rows and
    // stores 16 B per lane, 256 contiguous bytes per row - half the store instructions of writing
    // the accumulator layout directly, which is what bounds a store tail (T21). ----
    lgkm_wait0();
    __builtin_amdgcn_s_barrier();  // every wave is done with the ring (its last DMAs retired above)
    if constexpr (PERSIST) {
      // The one-tile epilogue below with the seam around it: staged in NP = 2 passes of RPP = 64 rows
      // (IPP 16-row blocks) per wave through half-slots 2 - 4, half-slots 0 and 1 taking the next
      // tile's A_0 and B_0 meanwhile.  The arithmetic of every kind is the one-tile form's, to the letter.
      static_assert(!PERSIST || EPI == TILE_EPI_SWIGLU8 || EPI == TILE_EPI_ROPE || EPI == TILE_EPI_RESID,
                    "the persistent epilogue has the kinds of kTilePersist");
      fresh_ids();
      constexpr bool SWG = EPI == TILE_EPI_SWIGLU8;
      constexpr int OUTW = SWG ? 64 : 128;  // output columns of this wave's quarter
      constexpr int RS_ = OUTW * 2 + 16;    // LDS row stride (16-B pad: 2-way writes)
      constexpr int NP = 2, RPP = 128 / NP, IPP = 8 / NP, SBASE = 2 * HS;
      char* stage = smem + SBASE + wave * (RPP * RS_);
      const int ml = lane & 15, nq = 4 * (lane >> 4);
      const int rr = lane >> 4, cc = lane & 15;
      uint4 nwv{};
      // RESID (N % 128 == 0): the wave's 128 columns are all inside N or, in a last n-tile of 128
      // columns, all past it - then it stores nothing (its offsets would alias the next row): branch-free,
      // its norm weights are read from the tile's first quarter and its offsets are out of range
      [[maybe_unused]] const bool quarter_in = nrows - wn * 128 >= 128;
      if constexpr (EPI == TILE_EPI_RESID)
        nwv = *reinterpret_cast<const uint4*>(ep.norm_w + n0 + (quarter_in ? wn * 128 : 0) + cc * 8);
      // RS: each thread's row scale through LDS (after the staging area) to the lanes holding the row
      float sc[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) sc[i] = 1.f;
      float* inv_s = reinterpret_cast<float*>(smem + SBASE + 4 * RPP * (128 * 2 + 16));
      if constexpr (RS) inv_s[tid] = rs_inv;
      // the seam, first half: the next tile's coordinates (nx) and DMA operands, its A_0 and B_0 into
      // half-slots 0 and 1
      vb += gridDim.x;
      more = vb < nwg;
      if (more) {
        nx = tile_of(vb);
        dma_setup(nx);
        issue_half(0, 0);
        issue_half(1, 0);
      }
      if constexpr (RS) {
        lgkm_wait0();  // a raw barrier: __syncthreads() would wait for the pieces in flight
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int i = 0; i < 8; ++i) sc[i] = inv_s[wm * 128 + i * 16 + ml];
      }
      // pass h: rows h RPP .. of the wave's quarter, at staging rows 0 ..
      auto epi_pass = [&](auto hc) {
        constexpr int h = decltype(hc)::value;
#pragma unroll
        for (int i = h * IPP; i < (h + 1) * IPP; ++i) {
          __builtin_amdgcn_sched_barrier(0);  // one row block's accumulators at a time (no hoisted AGPR reads)
          char* srow = stage + ((i - h * IPP) * 16 + ml) * RS_ + nq * 2;
          if constexpr (EPI == TILE_EPI_SWIGLU8) {
            const int hi = lane >> 5, qq = (lane >> 4) & 1;
            char* srow8 = stage + ((i - h * IPP) * 16 + ml) * RS_ + (8 * qq + 4 * hi);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              float g[4], u[4];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const uint32_t v = __float_as_uint(acc[i][j][r] * sc[i]);
                const auto pr = __builtin_amdgcn_permlane32_swap(v, v, false, false);
                g[r] = __uint_as_float(pr[0]);
                u[r] = __uint_as_float(pr[1]);
              }
              float o[2];
#pragma unroll
              for (int k = 0; k < 2; ++k) {
                const float gt = bf2f(f2bf(hi ? g[2 + k] : g[k])), up = bf2f(f2bf(hi ? u[2 + k] : u[k]));
                o[k] = gt * up / (1.f + __expf(-gt));
              }
              *reinterpret_cast<uint32_t*>(srow8 + j * 16) = pack2(o[0], o[1]);
            }
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const f32x4 v = acc[i][j] * sc[i];
              *reinterpret_cast<uint2*>(srow + j * 32) = uint2{pack2(v[0], v[1]), pack2(v[2], v[3])};
            }
          }
        }
        lgkm_wait0();
        // what the read-back of each kind needs, made per pass (scalars and a few lane offsets)
        // RESID: lane (rr, cc): row rr + 4b, columns cc*8 .. +7 of the wave's quarter; N % 128 == 0 (host)
        [[maybe_unused]] __amdgpu_buffer_rsrc_t rres, rhw;
        [[maybe_unused]] uint32_t ro = 0u;
        [[maybe_unused]] float wf[8];
        if constexpr (EPI == TILE_EPI_RESID) {
          rres = rsrc(ep.resid + (long)row0 * N, (long)mrows * N * 2);
          rhw = rsrc(ep.hw + (long)row0 * N, (long)mrows * N * 2);
          ro = quarter_in ? (uint32_t)(((wm * 128 + rr) * N + n0 + wn * 128 + cc * 8) * 2) : 0x80000000u;
          unpack8(nwv, wf);
        }
        [[maybe_unused]] const int ss_np = N >> 7, ssc = (n0 + wn * 128) >> 7;
        // ROPE: this wave's quarter is a rotated head; else its rows go out as they are
        [[maybe_unused]] const bool rot = EPI == TILE_EPI_ROPE && ((n0 + wn * 128) >> 7) < ep.rope_heads && nrows - wn * 128 >= 128;
        constexpr int CPR = OUTW / 8;  // 16-B chunks per row
        constexpr int RPI = 64 / CPR;  // rows per wave instruction
        const int ldy = SWG ? (N >> 1) : N;
        const int col0 = SWG ? ((n0 + wn * 128) >> 1) : n0 + wn * 128;
        const int ncols = SWG ? (nrows >> 1) - wn * 64 : nrows - wn * 128;
        const int rr2 = lane / CPR, cc2 = lane % CPR;
        // branch-free masked stores: a buffer descriptor over this m-tile's rows drops every store past
        // row mrows (out of range), and a lane whose columns are past N gets an out-of-range offset
        const __amdgpu_buffer_rsrc_t yr = rsrc(Y + (long)row0 * ldy, (long)mrows * ldy * 2);
        const uint32_t yo = cc2 * 8 < ncols ? (uint32_t)(((wm * 128 + rr2) * ldy + col0 + cc2 * 8) * 2) : 0x80000000u;
        if constexpr (EPI == TILE_EPI_RESID) {
#pragma unroll
          for (int b = h * (32 / NP); b < (h + 1) * (32 / NP); ++b) {
            const int r = rr + 4 * b;
            const uint4 yv = *reinterpret_cast<const uint4*>(stage + (r - h * RPP) * RS_ + cc * 16);
            float y[8], rv[8], hh[8], hw[8];
            unpack8(yv, y);
            const u32x4 rb = resq[b & 15];
            if (b < 16) resq[b] = __builtin_amdgcn_raw_buffer_load_b128(rres, ro + (uint32_t)(4 * (b + 16) * N * 2), 0, 0);
            unpack8(uint4{rb[0], rb[1], rb[2], rb[3]}, rv);
            float ss = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              hh[e] = bf2f(f2bf(y[e] + rv[e]));
              ss += hh[e] * hh[e];
              hw[e] = hh[e] * wf[e];
            }
            const uint4 hq = pack8(hh), wq = pack8(hw);
            const uint32_t off = ro + (uint32_t)(4 * b * N * 2);
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{hq.x, hq.y, hq.z, hq.w}, rres, off, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{wq.x, wq.y, wq.z, wq.w}, rhw, off, 0, 0);
            ss = row16_sum(ss);
            const int grow = wm * 128 + r;
            if (cc == 0 && grow < mrows && quarter_in) ep.ss_out[(long)(row0 + grow) * ss_np + ssc] = ss;
          }
        } else if (rot) {
          // one lane per (row, chunk pair c, c + 8): 8 rows per pass, 16 passes over the quarter's rows
          const int c = lane & 7, rsub = lane >> 3;
          bf16_t* ybase = Y + (long)row0 * N + n0 + wn * 128;
#pragma unroll 4
          for (int pass = h * (16 / NP); pass < (h + 1) * (16 / NP); ++pass) {
            const int r = pass * 8 + rsub, grow = wm * 128 + r;
            if (grow >= mrows) continue;
            const uint4 a = *reinterpret_cast<const uint4*>(stage + (r - h * RPP) * RS_ + c * 16);
            const uint4 b = *reinterpret_cast<const uint4*>(stage + (r - h * RPP) * RS_ + (c + 8) * 16);
            const float* cs = ep.cos_sin + (long)ep.positions[row0 + grow] * 128;
            const float4 c0 = *reinterpret_cast<const float4*>(cs + c * 8), c1 = *reinterpret_cast<const float4*>(cs + c * 8 + 4);
            const float4 s0 = *reinterpret_cast<const float4*>(cs + 64 + c * 8),
                         s1 = *reinterpret_cast<const float4*>(cs + 64 + c * 8 + 4);
            const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
            const float ss[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
            float x1[8], x2[8], o1[8], o2[8];
            unpack8(a, x1);
            unpack8(b, x2);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              o1[j] = x1[j] * cc[j] - x2[j] * ss[j];
              o2[j] = x2[j] * cc[j] + x1[j] * ss[j];
            }
            bf16_t* yrow = ybase + (long)grow * N;
            *reinterpret_cast<uint4*>(yrow + c * 8) = pack8(o1);
            *reinterpret_cast<uint4*>(yrow + 64 + c * 8) = pack8(o2);
          }
        } else {
#pragma unroll
          for (int b = h * (RPP / RPI); b < (h + 1) * (RPP / RPI); b += 8) {  // 8 row groups per batch: reads issued back to back
            u32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
              v[u] = *reinterpret_cast<const u32x4*>(stage + ((b + u) * RPI + rr2 - h * RPP) * RS_ + cc2 * 16);
#pragma unroll
            for (int u = 0; u < 8; ++u)
              __builtin_amdgcn_raw_buffer_store_b128(v[u], yr, yo + (uint32_t)((b + u) * RPI * ldy * 2), 0, 0);
          }
        }
      };
      epi_pass(std::integral_constant<int, 0>{});
      epi_pass(std::integral_constant<int, 1>{});
      // the seam, second half: once every wave has read its staging rows back (a wave's pieces land
      // in all of half-slots 2 - 4), A_1 B_1 A_2 - the 24 pieces the next tile's first wait leaves
      // in flight; this tile's stores drain under them
      if (more) {
        lgkm_wait0();
        __builtin_amdgcn_s_barrier();
        fresh_ids();
        dma_setup(nx);  // again: the lane offsets are not kept over the epilogue
        issue_half(0, 1);
        issue_half(1, 1);
        issue_half(0, 2);
        row0 = nx.row0;
        mrows = nx.mrows;
        n0 = nx.n0;
        nrows = nx.nrows;
      }
      first = false;
    } else {
      constexpr bool SWG = EPI == TILE_EPI_SWIGLU || EPI == TILE_EPI_SWIGLU8;
      constexpr int OUTW = SWG ? 64 : 128;  // output columns of this wave's quarter
      constexpr int RS_ = OUTW * 2 + 16;                       // LDS row stride (16-B pad: 2-way writes)
      char* stage = smem + wave * (128 * RS_);
      const int ml = lane & 15, nq = 4 * (lane >> 4);
      const int rr = lane >> 4, cc = lane & 15;
      uint4 nwv{};
      // RESID (N % 128 == 0): the wave's 128 columns are all inside N or, in a last n-tile of 128
      // columns, all past it - then it stores nothing (its offsets would alias the next row): branch-free,
      // its norm weights are read from the tile's first quarter and its offsets are out of range
      [[maybe_unused]] const bool quarter_in = nrows - wn * 128 >= 128;
      if constexpr (EPI == TILE_EPI_RESID)
        nwv = *reinterpret_cast<const uint4*>(ep.norm_w + n0 + (quarter_in ? wn * 128 : 0) + cc * 8);
      // RS: each thread's row scale through LDS (after the staging area) to the lanes holding the row
      float sc[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) sc[i] = 1.f;
      if constexpr (RS) {
        float* inv_s = reinterpret_cast<float*>(smem + 4 * 128 * (128 * 2 + 16));
        inv_s[threadIdx.x] = rs_inv;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) sc[i] = inv_s[wm * 128 + i * 16 + ml];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        __builtin_amdgcn_sched_barrier(0);  // one row block's accumulators at a time (no hoisted AGPR reads)
        char* srow = stage + (i * 16 + ml) * RS_ + nq * 2;
        if constexpr (EPI == TILE_EPI_SWIGLU) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float gt = bf2f(f2bf(acc[i][j][r] * sc[i])), up = bf2f(f2bf(acc[i][j + 4][r] * sc[i]));
              o[r] = gt * up / (1.f + __expf(-gt));
            }
            *reinterpret_cast<uint2*>(srow + j * 32) = uint2{pack2(o[0], o[1]), pack2(o[2], o[3])};
          }
        } else if constexpr (EPI == TILE_EPI_SWIGLU8) {
          // [8 gate | 8 up] per 16-column n-tile j: gate column 4 q + r (q = 0, 1: lanes 0-31) pairs
          // with up column 8 + 4 q + r in lane + 32.  One v_permlane32_swap per register puts (gate,
          // up) in both lane halves; lanes 0-31 finish r = 0, 1 and lanes 32-63 r = 2, 3 of feature
          // 8 j + 4 q + r (4 bytes each).
          const int hi = lane >> 5, qq = (lane >> 4) & 1;
          char* srow8 = stage + (i * 16 + ml) * RS_ + (8 * qq + 4 * hi);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float g[4], u[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const uint32_t v = __float_as_uint(acc[i][j][r] * sc[i]);
              const auto pr = __builtin_amdgcn_permlane32_swap(v, v, false, false);
              g[r] = __uint_as_float(pr[0]);
              u[r] = __uint_as_float(pr[1]);
            }
            float o[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              const float gt = bf2f(f2bf(hi ? g[2 + k] : g[k])), up = bf2f(f2bf(hi ? u[2 + k] : u[k]));
              o[k] = gt * up / (1.f + __expf(-gt));
            }
            *reinterpret_cast<uint32_t*>(srow8 + j * 16) = pack2(o[0], o[1]);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const f32x4 v = acc[i][j] * sc[i];
            *reinterpret_cast<uint2*>(srow + j * 32) = uint2{pack2(v[0], v[1]), pack2(v[2], v[3])};
          }
        }
      }
      lgkm_wait0();
      if constexpr (EPI == TILE_EPI_RESID) {
        // lane (rr, cc): row rr + 4b, columns cc*8 .. +7 of the wave's quarter; N % 128 == 0 (host)
        const __amdgpu_buffer_rsrc_t rres = rsrc(ep.resid + (long)row0 * N, (long)mrows * N * 2);
        const __amdgpu_buffer_rsrc_t rhw = rsrc(ep.hw + (long)row0 * N, (long)mrows * N * 2);
        const uint32_t ro = quarter_in ? (uint32_t)(((wm * 128 + rr) * N + n0 + wn * 128 + cc * 8) * 2) : 0x80000000u;
        float wf[8];
        unpack8(nwv, wf);
        const int ss_np = N >> 7, ssc = (n0 + wn * 128) >> 7;
#pragma unroll
        for (int b = 0; b < 32; ++b) {
          const int r = rr + 4 * b;
          const uint4 yv = *reinterpret_cast<const uint4*>(stage + r * RS_ + cc * 16);
          float y[8], rv[8], h[8], hw[8];
          unpack8(yv, y);
          const u32x4 rb = resq[b & 15];
          if (b < 16) resq[b] = __builtin_amdgcn_raw_buffer_load_b128(rres, ro + (uint32_t)(4 * (b + 16) * N * 2), 0, 0);
          unpack8(uint4{rb[0], rb[1], rb[2], rb[3]}, rv);
          float ss = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            h[e] = bf2f(f2bf(y[e] + rv[e]));
            ss += h[e] * h[e];
            hw[e] = h[e] * wf[e];
          }
          const uint4 hq = pack8(h), wq = pack8(hw);
          const uint32_t off = ro + (uint32_t)(4 * b * N * 2);
          __builtin_amdgcn_raw_buffer_store_b128(u32x4{hq.x, hq.y, hq.z, hq.w}, rres, off, 0, 0);
          __builtin_amdgcn_raw_buffer_store_b128(u32x4{wq.x, wq.y, wq.z, wq.w}, rhw, off, 0, 0);
          ss = row16_sum(ss);
          const int grow = wm * 128 + r;
          if (cc == 0 && grow < mrows && quarter_in) ep.ss_out[(long)(row0 + grow) * ss_np + ssc] = ss;
        }
        return;
      }
      if constexpr (EPI == TILE_EPI_ROPE) {
        const int head = (n0 + wn * 128) >> 7;
        if (head < ep.rope_heads && nrows - wn * 128 >= 128) {
          // one lane per (row, chunk pair c, c + 8): 8 rows per pass, 16 passes over the quarter's rows
          const int c = lane & 7, rsub = lane >> 3;
          bf16_t* ybase = Y + (long)row0 * N + n0 + wn * 128;
#pragma unroll 4
          for (int pass = 0; pass < 16; ++pass) {
            const int r = pass * 8 + rsub, grow = wm * 128 + r;
            if (grow >= mrows) continue;
            const uint4 a = *reinterpret_cast<const uint4*>(stage + r * RS_ + c * 16);
            const uint4 b = *reinterpret_cast<const uint4*>(stage + r * RS_ + (c + 8) * 16);
            const float* cs = ep.cos_sin + (long)ep.positions[row0 + grow] * 128;
            const float4 c0 = *reinterpret_cast<const float4*>(cs + c * 8), c1 = *reinterpret_cast<const float4*>(cs + c * 8 + 4);
            const float4 s0 = *reinterpret_cast<const float4*>(cs + 64 + c * 8),
                         s1 = *reinterpret_cast<const float4*>(cs + 64 + c * 8 + 4);
            const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
            const float ss[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
            float x1[8], x2[8], o1[8], o2[8];
            unpack8(a, x1);
            unpack8(b, x2);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              o1[j] = x1[j] * cc[j] - x2[j] * ss[j];
              o2[j] = x2[j] * cc[j] + x1[j] * ss[j];
            }
            bf16_t* yr = ybase + (long)grow * N;
            *reinterpret_cast<uint4*>(yr + c * 8) = pack8(o1);
            *reinterpret_cast<uint4*>(yr + 64 + c * 8) = pack8(o2);
          }
          return;
        }
      }
      constexpr int CPR = OUTW / 8;  // 16-B chunks per row
      constexpr int RPI = 64 / CPR;  // rows per wave instruction
      const int ldy = SWG ? (N >> 1) : N;
      const int col0 = SWG ? ((n0 + wn * 128) >> 1) : n0 + wn * 128;
      const int ncols = SWG ? (nrows >> 1) - wn * 64 : nrows - wn * 128;
      const int rr2 = lane / CPR, cc2 = lane % CPR;
      // branch-free masked stores: a buffer descriptor over this m-tile's rows drops every store past
      // row mrows (out of range), and a lane whose columns are past N gets an out-of-range offset
      const __amdgpu_buffer_rsrc_t yr = rsrc(Y + (long)row0 * ldy, (long)mrows * ldy * 2);
      const uint32_t yo = cc2 * 8 < ncols ? (uint32_t)(((wm * 128 + rr2) * ldy + col0 + cc2 * 8) * 2) : 0x80000000u;
#pragma unroll
      for (int b = 0; b < 128 / RPI; b += 8) {  // 8 row groups per batch: reads issued back to back
        u32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const u32x4*>(stage + ((b + u) * RPI + rr2) * RS_ + cc2 * 16);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          __builtin_amdgcn_raw_buffer_store_b128(v[u], yr, yo + (uint32_t)((b + u) * RPI * ldy * 2), 0, 0);
      }
    }
  } while (PERSIST && more);
}

}  // namespace k8sllm

using namespace k8sllm;

namespace {

struct TileLaunch {  // what every instantiation is launched with
  dim3 grid;
  hipStream_t s;
  const bf16_t *X, *W;
  bf16_t* Y;
  const int* offsets;
  int E, M, N, K;
  long w_es;
  int n_mt, n_nt;
  TileEpi ep;
  int wpk;
  const float* wscale;
};

// The walk over kTileForms from row F on: launches row `form` at schedule `sch` - each row is
// instantiated at schedule 1 and, where it says so, at schedule 0, and nothing else is.
template <int F = 0>
bool tile_dispatch(int form, int sch, const TileLaunch& l) {
  if constexpr (F == kTileNForms) {
    return false;
  } else {
    if (form != F) return tile_dispatch<F + 1>(form, sch, l);
    constexpr TileForm f = kTileForms[F];
    auto launch = [&](auto sc) {
      hipLaunchKernelGGL((gemm_w4_kernel<f.epi, f.grouped != 0, decltype(sc)::value, f.rs != 0, f.fmt == TILE_W_F8,
                                         f.fmt == TILE_W_F4>),
                         l.grid, dim3(256), 0, l.s, l.X, l.W, l.Y, l.offsets, l.E, l.M, l.N, l.K, l.w_es, l.n_mt,
                         l.n_nt, l.ep, l.wpk, l.wscale);
      return true;
    };
    if constexpr (f.sch0 != 0)
      if (sch == 0) return launch(std::integral_constant<int, 0>{});
    return sch == 1 && launch(std::integral_constant<int, 1>{});
  }
}

// The same over kTilePersist: row `pi`, the PERSIST instantiation (dense bf16 W, schedule 1).
template <int P = 0>
bool tile_dispatch_persist(int pi, const TileLaunch& l) {
  if constexpr (P == kTileNPersist) {
    return false;
  } else {
    if (pi != P) return tile_dispatch_persist<P + 1>(pi, l);
    constexpr TilePersistForm f = kTilePersist[P];
    hipLaunchKernelGGL((gemm_w4_kernel<f.epi, false, 1, f.rs != 0, false, false, true>), l.grid, dim3(256), 0, l.s, l.X,
                       l.W, l.Y, l.offsets, l.E, l.M, l.N, l.K, l.w_es, l.n_mt, l.n_nt, l.ep, l.wpk, l.wscale);
    return true;
  }
}

// The device's CU count, asked once per device.
int tile_cus() {
  static int cus[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return kTileCUs;
  if (cus[dev] == 0) {
    int n = 0;
    cus[dev] = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : kTileCUs;
  }
  return cus[dev];
}

}  // namespace

// THE launcher of gemm_w4_kernel; what it accepts, the schedule that runs and the grid are
// tile_plan's (gemm_tile_forms.h, with the table of accepted launches).
// Dense (offsets == nullptr): Y [M][N] (SwiGLU: [M][N / 2]) = X [M][K] . W[N][K]^T.
// Grouped: W [E][N][K] with expert stride w_es elements; M = total expert-sorted rows (the grid
// bound: ceil(M / 256) + E m-tiles); expert e's rows are offsets[e] .. offsets[e + 1] - 1.
// W by wfmt: 0 bf16, row-major or (wpk) fragment-packed [E][N/16][K/32][64][8] (ops.pack_skinny - the
// decode GEMMs' layout: every W DMA piece is one contiguous 1-KiB block, read lane-linear from LDS),
// wscale null; 1 fp8, e4m3 codes [N/16][K/64][64][16] (ops.pack_skinny_f8) with wscale [N] fp32 row
// scales in packed row order; 2 mxfp4, e2m1 codes [N/16][K/128][64][16] with wscale the e8m0 block
// scales [N/16][K/128][16][4] bytes (ops.pack_skinny_f4).
// persist / cus: tile_plan's (A/B runs): -1 = the persistent form where the table routes it, 1 = wherever
// it is compiled, 0 = nowhere; cus 0 = the device's CU count, else the persistent grid's size.
// Returns 0 or tile_plan's negative code; a wfmt / wscale mismatch is -4, a missing epilogue operand -1.
extern "C" int k8sllm_gemm_tile(const void* X, const void* W, void* Y, int M, int N, int K, const int* offsets, int E,
                                long w_es, int epi, int algo, const int* rope_pos, const float* rope_cs,
                                int rope_heads, const float* rs_part, int rs_np, float rs_eps, void* resid, void* hw,
                                const void* norm_w, float* ss_out, int wpk, const void* wscale, int wfmt, int persist,
                                int cus, hipStream_t s) {
  const TilePlan p = tile_plan((wfmt != 0) == (wscale != nullptr) ? wfmt : -1, M, N, K, epi, algo,
                               tile_count_arg(offsets != nullptr, E), tile_count_arg(rs_part != nullptr, rs_np),
                               persist, cus > 0 ? cus : persist != 0 ? tile_cus() : 0);
  if (M <= 0 || p.err == -4) return p.err;
  if (epi == TILE_EPI_ROPE && (rope_pos == nullptr || rope_cs == nullptr)) return -1;
  if (epi == TILE_EPI_RESID && (resid == nullptr || hw == nullptr || norm_w == nullptr || ss_out == nullptr)) return -1;
  if (p.err < 0) return p.err;
  const TileLaunch l{dim3((unsigned)p.grid), s, (const bf16_t*)X, (const bf16_t*)W, (bf16_t*)Y, offsets, E, M, N, K,
                     w_es, p.n_mt, p.n_nt,
                     TileEpi{rope_pos, rope_cs, rope_heads, rs_part, rs_np, rs_eps, (bf16_t*)resid, (bf16_t*)hw,
                             (const bf16_t*)norm_w, ss_out},
                     wpk, (const float*)wscale};
  if (!(p.persist >= 0 ? tile_dispatch_persist(p.persist, l) : tile_dispatch(p.form, p.sch, l))) return -1;
  return (int)hipGetLastError();
}

// The rows of kTilePersist as three ints each (epi, rs, on), at most cap rows into out; returns the row count.
extern "C" int k8sllm_gemm_tile_persist_forms(int* out, int cap) {
  for (int i = 0; i < kTileNPersist && i < cap; ++i) {
    out[3 * i] = kTilePersist[i].epi;
    out[3 * i + 1] = kTilePersist[i].rs;
    out[3 * i + 2] = kTilePersist[i].on;
  }
  return kTileNPersist;
}

// The rows of kTileForms as five ints each (weight format, epi, grouped, rs, sch0), at most cap
// rows into out; returns the row count.
extern "C" int k8sllm_gemm_tile_forms(int* out, int cap) {
  for (int i = 0; i < kTileNForms && i < cap; ++i) {
    const TileForm& f = kTileForms[i];
    const int row[5] = {f.fmt, f.epi, f.grouped, f.rs, f.sch0};
    for (int j = 0; j < 5; ++j) out[5 * i + j] = row[j];
  }
  return kTileNForms;
}
