// Decode-time GEMM, second design ("W stream, shared A"): Y[M, N] = A[M, K] . W[N, K]^T for
// M <= 128 rows (dense launches; grouped launches and the row-complete kernel M <= 64), bf16 in,
// fp32 accumulate, gfx950 v_mfma_f32_16x16x32_bf16.  The compiled forms and the row limits:
// kDecForms in gemm_dec_forms.h.
//
// Why a second kernel.  gemm_skinny_rm_kernel (gemm_skinny.hip) stages BOTH operands by LDS-DMA,
// and at M = 64 every 64-column workgroup re-reads all 64 A rows - as many bytes as its weight
// slab.  The round-2 PMC reading (profiles/r02/README.md "Why the row-major skinny GEMM loses
// weight bandwidth") put the vector-memory path at 84-88 % busy moving ~16 B/cycle/CU of W + A,
// half of it A, and the decode GEMMs at 3.4-4.8 TB/s against 5.9-6.2 at M = 1.  Here:
//   * W is a decode-only fragment-packed copy [N/16][K/32][64][8] (pack_skinny): every wave
//     instruction is 1 KiB contiguous straight into MFMA operand registers (global_load_dwordx4,
//     non-temporal: read once per step), no LDS round trip, and each wave keeps DEPTH k-steps of
//     its weight stream in flight in a register ring;
//   * A (fragment-packed activations) is loaded ONCE per workgroup per K chunk into LDS (register
//     staged: global_load -> ds_write_b128, a 2-slot ring, one barrier per chunk) and read by
//     every wave - the waves split the workgroup's COLUMNS, not K, so A bytes per weight byte are
//     MT / (n-tiles per workgroup) instead of MT / 4;
//   * the grid is sized to the chip: n-tiles per workgroup x split-K chosen so the workgroup count
//     is ~256 (one per CU, every CU the same weight bytes; e.g. gate_up: 1792 n-tiles / 7 = 256);
//   * no cross-wave combine: each wave owns whole-K sums of its columns.
// Epilogues: SLAB (fp32 split-K partials [S][M][N] for the next kernel's reduce, as the skinny
// kernels), BF16 (the LM head), SWIGLU8 (gate_up with the weight rows interleaved per 16-row
// n-tile as [8 gate | 8 up]: the pair sits in lanes l and l ^ 8 of the same accumulator, so the
// epilogue is one lane swap; output fragment-packed as the down projection's A operand).
#include <type_traits>

#include "common.h"
#include "gemm_dec_forms.h"

namespace k8sllm {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Grouped launches (MoE experts, grid.z = local expert e): A, W and the SWIGLU8 output advance by
// a per-expert stride; SLAB partials land in slab e * S + split, scaled by the routing weight
// rw[row * rw_ld + e] (0 where the row did not pick the expert), so the residual-add kernel's slab
// sum IS the expert combine.  Dense launches: all strides 0, rw null, grid.z 1.
// The weight stride is in BYTES: the stack holds bf16 (2 B per element), e4m3 codes (1 B) or
// packed e2m1 codes (1/2 B), and the scales of a quantised stack ride beside it with a byte
// stride of their own (fp8: N fp32 row scales per expert; mxfp4: (N/16)(K/128) 16 block-scale
// dwords).
struct DecGroup {
  long a_es, y_es;  // elements between experts' A / SWIGLU8 outputs
  long w_eb, s_eb;  // bytes between experts' weights / their scales (s_eb: quantised stacks)
  const float* rw;        // [M][rw_ld] routing weights (SLAB epilogue) or null
  int rw_ld;
  // Pre-activation delta of a dense SWIGLU8 launch (the adapters' gate_up delta, ops.lora_slab), or
  // null: delta [M][N] fp32 over the packed row index, added to the rows whose dslot[row] names an
  // adapter of the arena (0 <= slot < nslots) before gate and up are rounded to bf16.
  const float* delta;
  const int* dslot;
  int nslots;
};

// v + d as two roundings: v (a product the compiler holds in a register) is pinned first, so the
// add is never contracted into an fma with the factors of v.  The fp8 launch multiplies the
// accumulator by the row's power-of-two scale and the bf16 launch over the dequantised weights does
// not: fused, the two would round differently.
__device__ __forceinline__ float dec_add_delta(float v, float d) {
  asm volatile("" : "+v"(v));
  return v + d;
}

// One lane's part of the SWIGLU8 store: v is this lane's pre-activation (gate in lanes with
// l & 8 == 0, the matching up in lane l ^ 8); gate and up are rounded to bf16 first, as the unfused
// GEMM -> silu_mul does, and the gate lane stores feature f of `row` fragment-packed.
__device__ __forceinline__ void dec_swiglu_store(bf16_t* __restrict__ Y, int F, int f, int row, int lane, float v) {
  const float o = __shfl_xor(v, 8, kWave);
  if ((lane & 8) == 0) {
    const float g = bf2f(f2bf(v)), u = bf2f(f2bf(o));
    Y[(((long)(row >> 4) * (F >> 5) + (f >> 5)) * 64 + ((f >> 3) & 3) * 16 + (row & 15)) * 8 + (f & 7)] =
        f2bf(g * u / (1.f + __expf(-g)));
  }
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t dec_rsrc(const void* base, long bytes) {
  const uint64_t a = reinterpret_cast<uint64_t>(base);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  const int nb = __builtin_amdgcn_readfirstlane((int)min(bytes, 0x7fffffffL));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, nb, 0x00020000);
}
constexpr int kRnMax = 4;   // narrow deferred-norm rows: up to 16 partials (4 per thread)
constexpr int kRnWide = 16;  // wide rows: up to 256 partials (16 x 16 B per thread)

constexpr int kDecCH = 8;  // k-steps (32 deep) per A chunk
constexpr int kDecSC1 = 16;  // buffer-op aux bits: sc1 (write-through stores)

template <int MT, int WAVES>
struct DecGeom {
  static constexpr int SLOT = kDecCH * MT * 1024;                   // bytes of one A chunk
  static constexpr int PIECES = kDecCH * MT * 64;                   // 16-B pieces per chunk
  static constexpr int NLD = (PIECES + 64 * WAVES - 1) / (64 * WAVES);  // staging loads per thread
};

// 8 OCP e4m3 codes (two dwords, the first code in the low byte) -> the bf16x8 MFMA operand, unscaled:
// four v_cvt_scalef32_pk_bf16_fp8.  Exact: every finite e4m3 value is a bf16 value.
__device__ __forceinline__ bf16x8 dec_f8x8(uint32_t lo, uint32_t hi) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
  return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// 8 e2m1 codes (one dword: element 2i in the low nibble of byte i) times the block scale (an fp32
// power of two) -> the bf16x8 MFMA operand: four v_cvt_scalef32_pk_bf16_fp4, one per byte.  Exact:
// code * 2^e is a bf16 value for |e| <= 60.
__device__ __forceinline__ bf16x8 dec_f4x8(uint32_t q, float scale) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 0);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 1);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 2);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 3);
  return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// WF, the weight format: DEC_W_BF16, DEC_W_F8 or DEC_W_F4.
// F8: W holds e4m3 codes [N/16][K/64][64][16] (pack_skinny_f8: lane l's 16 bytes are its 8 codes of
// k-step 2j, then its 8 of k-step 2j + 1, in the bf16 layout's fragment order), so one 1-KiB wave
// load feeds two k-steps and the ring holds DEPTH / 2 loads per n-tile.  A fragment is converted
// once per (k-step, n-tile), unscaled, and runs the bf16 MFMA sequence in the bf16 order; the
// weight row's power-of-two scale wscale[packed row] multiplies the fp32 accumulator in the
// epilogue (after the deferred-norm row scale, before the routing weight of a grouped launch and
// before any bf16 rounding), which commutes with every rounding: bit-identical to the bf16 launch
// over the dequantised weights.  The narrow deferred norm only.
// F4: W holds MXFP4 (e2m1) codes [N/16][K/128][64][16] (pack_skinny_f4: lane l's dword s is its 8
// codes of k-step 4g + s, in the bf16 layout's fragment order), so one 1-KiB wave load feeds four
// k-steps and the ring holds DEPTH / 4 loads per n-tile (DEPTH here is the F4 ring depth the
// launcher chose - 8, or at one m-tile the F4 table's 16 - not the form's).  The block scales
// ride beside them: wscale is [N/16][K/128][16] dwords, dword (tile, g, r) the four e8m0 bytes of
// row r for k-steps 4g .. 4g + 3 (byte b is the fp32 b << 23); one 64-byte wave load per ring
// slot, issued with the slot's code load.  A fragment is converted
// once per (k-step, n-tile) WITH its block scale and runs the bf16 MFMA sequence in the bf16
// order; the epilogue is the bf16 one.  The narrow deferred norm only.
template <int MT, int NTW, int WAVES, int EPI, int DEPTH, bool RNW = false, int WF = DEC_W_BF16>
__global__ __launch_bounds__(64 * WAVES, 1) void gemm_dec_kernel(
    const bf16_t* __restrict__ A, const bf16_t* __restrict__ W, float* __restrict__ partial,
    bf16_t* __restrict__ Y, long ldy, int M, int N, int K, int kchunk, const float* __restrict__ rn_ss, int rn_nc,
    float rn_inv_d, float rn_eps, DecGroup grp, const float* __restrict__ wscale, int flags) {
  constexpr bool F8 = WF == DEC_W_F8, F4 = WF == DEC_W_F4;
  static_assert(!F8 || (!RNW && DEPTH % 2 == 0), "fp8 weights: narrow deferred norm, whole k-step pairs in the ring");
  static_assert(!F4 || (!RNW && DEPTH % 4 == 0), "mxfp4 weights: narrow deferred norm, whole k-step quads in the ring");
  using G = DecGeom<MT, WAVES>;
  const int ex = blockIdx.z;  // expert of a grouped launch (0 otherwise)
  A += ex * grp.a_es;
  W = reinterpret_cast<const bf16_t*>(reinterpret_cast<const char*>(W) + ex * grp.w_eb);
  if constexpr (F8 || F4) wscale = reinterpret_cast<const float*>(reinterpret_cast<const char*>(wscale) + ex * grp.s_eb);
  if constexpr (EPI == DEC_SWIGLU8) Y += ex * grp.y_es;
  constexpr int ITER = DEPTH > kDecCH ? DEPTH : kDecCH;  // k-steps per unrolled main-loop iteration
  __shared__ __attribute__((aligned(16))) char sA[2 * G::SLOT];
  __shared__ float s_inv[MT * 16];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ksteps = K >> 5;
  // (column group, split) of this workgroup.  kDecXcd (dense SLAB launches of 2, 4 or 8 splits whose
  // workgroup count is a multiple of 8: dec_plan): workgroups with equal linear id mod 8 - the ones
  // the dispatcher is observed to deal to one XCD - take the same split, so an XCD's L2 fetches
  // one split's A slice instead of all of them.  A bijection onto the same (x, y) set
  // (dec_xcd_map): placement is only ever a speed guess.
  int bx = blockIdx.x, by = blockIdx.y;
  if constexpr (EPI == DEC_SLAB) {
    if (flags & kDecXcd) {
      const DecXY m = dec_xcd_map(blockIdx.x + gridDim.x * blockIdx.y, gridDim.y);
      bx = m.x;
      by = m.y;
    }
  }
  const int kb = by * (kchunk >> 5);  // first k-step of this workgroup's K slice
  const int nsteps = kchunk >> 5;             // host: kchunk | K, (kchunk / 32) % ITER == 0
  const int niter = nsteps / ITER;
  const int tile0 = (bx * WAVES + wave) * NTW;  // this wave's first n-tile

  // ---- weight stream: DEPTH k-steps x NTW fragments in flight per wave, filled after chunk 0's
  // staging loads (below)
  // (F8: one load = a pair of k-steps; kb and DEPTH are even, so pairs never straddle a slice)
  // (F4: one load = four k-steps; kb and DEPTH are multiples of 4)
  constexpr int WSH = F4 ? 2 : F8 ? 1 : 0;
  constexpr int RING = DEPTH >> WSH;
  const int wsteps = ksteps >> WSH, wkb = kb >> WSH;
  const u32x4* wp[NTW];
#pragma unroll
  for (int t = 0; t < NTW; ++t)
    wp[t] = reinterpret_cast<const u32x4*>(W) + ((long)min(tile0 + t, (N >> 4) - 1) * wsteps + wkb) * 64 + lane;
  // F8: the scales of this lane's output columns, the oldest loads in flight (waited for once,
  // below the ring's first loads)
  float wsc[F8 ? NTW : 1];
  if constexpr (F8) {
#pragma unroll
    for (int t = 0; t < NTW; ++t) wsc[t] = wscale[min(tile0 + t, (N >> 4) - 1) * 16 + (lane & 15)];
  }
  // F4: the block scales of the ring's slots, a dword (four k-steps of row lane & 15) per slot
  const uint32_t* sp[F4 ? NTW : 1];
  if constexpr (F4) {
#pragma unroll
    for (int t = 0; t < NTW; ++t)
      sp[t] = reinterpret_cast<const uint32_t*>(wscale) + ((long)min(tile0 + t, (N >> 4) - 1) * wsteps + wkb) * 16 + (lane & 15);
  }
  u32x4 wr[RING][NTW];
  uint32_t wsr[F4 ? RING : 1][F4 ? NTW : 1];
  auto ring_fill = [&]() {
#pragma unroll
    for (int d = 0; d < RING; ++d)
#pragma unroll
      for (int t = 0; t < NTW; ++t) {
        wr[d][t] = __builtin_nontemporal_load(wp[t] + d * 64);
        if constexpr (F4) wsr[d][t] = __builtin_nontemporal_load(sp[t] + d * 16);
      }
  };

  // ---- the A rows' partial sums of squares (deferred RMSNorm), 4 threads per row, loaded first so
  // their wait below is a counted one.  Narrow rows (<= 16 partials:
  // add_norm_partial's per-512-column sums) one float per load; wide rows (16 | partials <= 256:
  // gemm_dec_rc_kernel's per-16-column sums) 16-byte loads, each thread a quarter of the row.
  // (RNW: the wide form, a compile-time choice - the host picks the instantiation by rn_nc)
  // Above 64 rows the MT * 64 row-threads outnumber a 4-, 6- or 7-wave workgroup (and equal an
  // 8-wave one): RNP passes over the rows, pass q taking row-thread threadIdx.x + q * 64 * WAVES,
  // so every one of the MT * 16 entries of s_inv is written whatever WAVES is.  RNP == 1 for
  // MT <= 4: the single pass of the 64-row kernel.
  constexpr int RNP = (MT * 64 + 64 * WAVES - 1) / (64 * WAVES);
  static_assert(!RNW || RNP == 1, "the wide deferred-norm form serves <= 64 rows (behind gemm_dec_rc)");
  float rnv[RNP][kRnMax];  // no initial value: read only under the same condition (no join wait)
  f32x4 rnw[RNW ? kRnWide : 1];
  const bool rn_narrow = !RNW && rn_nc <= 4 * kRnMax, rn_wide = RNW && rn_nc % 16 == 0 && rn_nc <= 16 * kRnWide;
  if constexpr (RNP > 1) {
    if (rn_ss != nullptr && rn_narrow) {
      const __amdgpu_buffer_rsrc_t ss_rs = dec_rsrc(rn_ss, (long)M * rn_nc * 4);
#pragma unroll
      for (int q = 0; q < RNP; ++q) {
        // row-threads past MT * 64 repeat row M - 1: every load unconditional and in bounds
        const int rt = threadIdx.x + q * 64 * WAVES;
        const int row = min(rt >> 2, M - 1), part = rt & 3;
#pragma unroll
        for (int j = 0; j < kRnMax; ++j) {
          const uint32_t off = (uint32_t)((row * rn_nc + min(part + 4 * j, rn_nc - 1)) * 4);
          rnv[q][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ss_rs, off, 0, 0));
        }
      }
    }
  } else if (rn_ss != nullptr && threadIdx.x < MT * 64 && (rn_narrow || rn_wide)) {
    const int row = min((int)(threadIdx.x >> 2), M - 1), part = threadIdx.x & 3;
    const __amdgpu_buffer_rsrc_t ss_rs = dec_rsrc(rn_ss, (long)M * rn_nc * 4);
    if constexpr (!RNW) {
#pragma unroll
      for (int j = 0; j < kRnMax; ++j) {
        const uint32_t off = (uint32_t)((row * rn_nc + min(part + 4 * j, rn_nc - 1)) * 4);
        rnv[0][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ss_rs, off, 0, 0));
      }
    } else {
      const int q = rn_nc >> 2;  // this thread's quarter: floats part*q .. part*q + q - 1
#pragma unroll
      for (int j = 0; j < (RNW ? kRnWide : 1); ++j) {
        const uint32_t off = (uint32_t)((row * rn_nc + part * q + min(4 * j, q - 4)) * 4);
        rnw[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ss_rs, off, 0, 0));
      }
    }
  }

  // ---- A chunks: register-staged, 2 LDS slots
  u32x4 stg[G::NLD];
  auto stage_load = [&](int c) {
#pragma unroll
    for (int i = 0; i < G::NLD; ++i) {
      // threads past the chunk (waves that do not divide it) repeat its last piece: every load
      // unconditional, so the counted vmcnt waits stay exact
      const int p = min((int)threadIdx.x + i * 64 * WAVES, G::PIECES - 1);
      const int mt = p / (kDecCH * 64), j = (p >> 6) % kDecCH, ln = p & 63;
      const long e = (((long)mt * ksteps + kb + c * kDecCH + j) * 64 + ln) * 8;
      stg[i] = *reinterpret_cast<const u32x4*>(A + e);
    }
  };
  auto stage_store = [&](int c) {
    char* slot = sA + (c & 1) * G::SLOT;
#pragma unroll
    for (int i = 0; i < G::NLD; ++i) {
      const int p = min((int)threadIdx.x + i * 64 * WAVES, G::PIECES - 1);
      *reinterpret_cast<u32x4*>(slot + p * 16) = stg[i];
    }
  };

  // chunk 0's staging loads go out BEFORE the weight ring's first loads: at the loop head the
  // staging registers are then the oldest loads in flight on both entry paths (prologue and back
  // edge), so the counted vmcnt there leaves the weight ring in flight (with the staging loads
  // last, the merged wait drained the ring at every chunk boundary).
  stage_load(0);
  ring_fill();
  if constexpr (F8) {
#pragma unroll
    for (int t = 0; t < NTW; ++t) asm volatile("" : "+v"(wsc[t]));  // a counted wait here, none in the epilogue
  }

  // ---- deferred RMSNorm: 1/rms of each A row from its partial sums of squares (loads issued
  // above, ahead of the A staging and the weight ring, so this wait leaves both in flight)
  if constexpr (RNP > 1) {
    if (rn_ss != nullptr) {
#pragma unroll
      for (int q = 0; q < RNP; ++q) {
        const int rt = threadIdx.x + q * 64 * WAVES;
        const int rl = rt >> 2, part = rt & 3;
        float ss = 0.f;
        if (rn_narrow) {
#pragma unroll
          for (int j = 0; j < kRnMax; ++j) {
            asm volatile("" : "+v"(rnv[q][j]));  // the first use (and its wait) stays past the ring issue
            ss += part + 4 * j < rn_nc ? rnv[q][j] : 0.f;
          }
        } else {  // other widths: a plain loop (no decode GEMM today)
          const int row = min(rl, M - 1);
          for (int c = part; c < rn_nc; c += 4) ss += rn_ss[row * rn_nc + c];
        }
        // 64 * WAVES is a multiple of 4: the 4 threads of a row sit in one wave in every pass
        ss += __shfl_xor(ss, 1, kWave);
        ss += __shfl_xor(ss, 2, kWave);
        if (part == 0 && rl < MT * 16) s_inv[rl] = rsqrtf(ss * rn_inv_d + rn_eps);
      }
    }
  } else if (rn_ss != nullptr && threadIdx.x < MT * 64) {
    const int rl = threadIdx.x >> 2, part = threadIdx.x & 3;
    float ss = 0.f;
    if (rn_narrow) {
#pragma unroll
      for (int j = 0; j < kRnMax; ++j) {
        asm volatile("" : "+v"(rnv[0][j]));  // keeps the first use (and its wait) here, past the ring issue
        ss += part + 4 * j < rn_nc ? rnv[0][j] : 0.f;
      }
    } else if (rn_wide) {
      const int q = rn_nc >> 2;
#pragma unroll
      for (int j = 0; j < (RNW ? kRnWide : 1); ++j) {
        asm volatile("" : "+v"(rnw[j][0]), "+v"(rnw[j][1]), "+v"(rnw[j][2]), "+v"(rnw[j][3]));
        if (4 * j < q) ss += (rnw[j][0] + rnw[j][1]) + (rnw[j][2] + rnw[j][3]);
      }
    } else {  // other widths: a plain loop (no decode GEMM today)
      const int row = min(rl, M - 1);
      for (int c = part; c < rn_nc; c += 4) ss += rn_ss[row * rn_nc + c];
    }
    ss += __shfl_xor(ss, 1, kWave);
    ss += __shfl_xor(ss, 2, kWave);
    if (part == 0) s_inv[rl] = rsqrtf(ss * rn_inv_d + rn_eps);
  }

  f32x4 acc[MT][NTW];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < NTW; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunks = nsteps / kDecCH;
  auto read_a = [&](bf16x8 (&af)[MT], int ks) {
    const char* slot = sA + ((ks / kDecCH) & 1) * G::SLOT + (ks % kDecCH) * 1024 + lane * 16;
#pragma unroll
    for (int m = 0; m < MT; ++m) af[m] = *reinterpret_cast<const bf16x8*>(slot + m * kDecCH * 1024);
  };
  // One unrolled iteration = ITER k-steps (a whole number of A chunks and of W ring turns).
  // Program order is pinned per k-step (sched_barrier): vmcnt retires in issue order, so a weight
  // load the scheduler sinks below the next chunk's staging loads would be drained at the next
  // chunk boundary and the ring would hold nothing across it.  Per k-step: the next step's A
  // fragments are read from LDS (one step of LDS latency hidden), the MFMAs consume ring slot
  // j % DEPTH, and the slot is refilled with k-step ks + DEPTH.  LAST: the final iteration issues
  // no weight loads past the slice.
  bf16x8 af[MT], an[MT];
  auto iteration = [&](int it, auto last) {
    constexpr bool LAST = decltype(last)::value;
#pragma unroll
    for (int j = 0; j < ITER; ++j) {
      const int ks = it * ITER + j;
      if (j % kDecCH == 0) {  // chunk boundary: publish chunk c, start loading chunk c + 1
        const int c = ks / kDecCH;
        stage_store(c);
        __syncthreads();
        if (c + 1 < nchunks) stage_load(c + 1);
        read_a(af, ks);
        __builtin_amdgcn_sched_barrier(0);
      } else {
#pragma unroll
        for (int m = 0; m < MT; ++m) af[m] = an[m];
      }
      if ((j + 1) % kDecCH != 0) read_a(an, ks + 1);
#pragma unroll
      for (int t = 0; t < NTW; ++t) {
        bf16x8 b;
        if constexpr (F8) {
          const u32x4 q = wr[(j % DEPTH) >> 1][t];
          b = (j & 1) ? dec_f8x8(q[2], q[3]) : dec_f8x8(q[0], q[1]);
        } else if constexpr (F4) {
          // the slot's code load and scale load are consumed together: one counted wait per slot
          const uint32_t e8 = (wsr[(j % DEPTH) >> 2][t] >> (8 * (j & 3))) & 0xffu;
          b = dec_f4x8(wr[(j % DEPTH) >> 2][t][j & 3], __uint_as_float(e8 << 23));
        } else {
          b = __builtin_bit_cast(bf16x8, wr[j % DEPTH][t]);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m], b, acc[m][t], 0, 0, 0);
      }
      if constexpr (F8) {
        if ((j & 1) && (!LAST || j + DEPTH < ITER)) {  // both k-steps of the slot consumed: the pair DEPTH ahead
#pragma unroll
          for (int t = 0; t < NTW; ++t)
            wr[(j % DEPTH) >> 1][t] = __builtin_nontemporal_load(wp[t] + ((ks + DEPTH) >> 1) * 64);
        }
      } else if constexpr (F4) {
        if ((j & 3) == 3 && (!LAST || j + DEPTH < ITER)) {  // the slot's four k-steps consumed: the quad DEPTH ahead
#pragma unroll
          for (int t = 0; t < NTW; ++t) {
            wr[(j % DEPTH) >> 2][t] = __builtin_nontemporal_load(wp[t] + ((ks + DEPTH) >> 2) * 64);
            wsr[(j % DEPTH) >> 2][t] = __builtin_nontemporal_load(sp[t] + ((ks + DEPTH) >> 2) * 16);
          }
        }
      } else if (!LAST || j + DEPTH < ITER) {
#pragma unroll
        for (int t = 0; t < NTW; ++t) wr[j % DEPTH][t] = __builtin_nontemporal_load(wp[t] + (ks + DEPTH) * 64);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  int it = 0;
  for (; it + 1 < niter; ++it) iteration(it, std::false_type{});
  iteration(it, std::true_type{});

  // ---- epilogue.  C layout of a 16x16 tile: col = lane & 15, rows (lane >> 4) * 4 + r.
  if constexpr (EPI == DEC_SLAB && MT > 1) {
    if (flags & kDecRows) {
      // Row-wide slab stores (two m-tiles and up: at one the 4-byte stores below are as fast or
      // faster, profiles/r24/README.md, and the one-m-tile kernels stay free of this path).  The
      // A ring is dead after the last k-step: every wave parks the values the 4-byte path stores
      // (same factors, same order: bit-identical slabs) in a padded row image
      // [MT * 16][16 NTW WAVES + 4] there, and each thread then stores 16-byte pieces of whole
      // rows - at 8 waves a wave instruction writes two 512-byte row segments, every 128-byte
      // line whole.  Banks: a ds_write_b32's 32-lane half holds two 4-row lane groups,
      // 4 LD = 16 (mod 32) dwords apart, so its 32 lanes hit 32 banks; a ds_read_b128's 16-lane
      // group reads 16 distinct 16-byte slots of one row at 8 waves (at 6 and 4 waves a group
      // that straddles two rows pays one 2-way conflict: the pad shifts the second row by a slot).
      constexpr int COLS = 16 * NTW * WAVES, LD = COLS + 4, PPR = COLS / 4;  // PPR: 16-byte pieces per row
      static_assert(MT * 16 * LD * 4 <= 2 * G::SLOT, "the row image fits the dead A ring");
      static_assert((MT * 16 * PPR) % (64 * WAVES) == 0, "whole passes of the workgroup over the image");
      float* img = reinterpret_cast<float*>(sA);
      __syncthreads();  // other waves may still be reading A fragments
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NTW; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int rl = m * 16 + (lane >> 4) * 4 + r;
            float v = acc[m][t][r] * (rn_ss != nullptr ? s_inv[rl] : 1.f);
            if constexpr (F8) v *= wsc[t];
            if (grp.rw != nullptr && rl < M) v = v * grp.rw[(long)rl * grp.rw_ld + ex];
            img[rl * LD + (wave * NTW + t) * 16 + (lane & 15)] = v;
          }
      __syncthreads();
      // this workgroup's slab: rows x N fp32 (dec_plan: under 2 GiB), columns col0 .. col0 + COLS - 1
      // as far as N reaches (the ragged last workgroup).  Buffer stores: rows at or past M are
      // also past the descriptor's range.
      const __amdgpu_buffer_rsrc_t rs = dec_rsrc(partial + (long)(ex * gridDim.y + by) * M * N, (long)M * N * 4);
      const int col0 = bx * COLS;
#pragma unroll
      for (int q0 = 0; q0 < MT * 16 * PPR; q0 += 64 * WAVES) {
        const int q = q0 + threadIdx.x;
        const int row = q / PPR, c = (q % PPR) * 4;
        if (row < M && col0 + c < N) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(img + row * LD + c);
          const uint32_t off = (uint32_t)((row * N + col0 + c) * 4);
          // write-through (kDecWt): the line leaves L2 as it is written, not at the kernel's end
          if (flags & kDecWt)
            __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, kDecSC1);
          else
            __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, 0);
        }
      }
      return;
    }
  }
  if constexpr (EPI == DEC_SWIGLU8) {
    if (grp.delta != nullptr) {
      // The SWIGLU8 epilogue with a pre-activation delta (host: a dense launch, narrow deferred
      // norm, M * N * 4 under 2 GiB).  A row's slot follows lora.hip's row_slot: rows past M and
      // slots outside the arena have no adapter.  The delta loads are buffer loads, all issued
      // before the first is used; a lane whose row has no adapter (or whose n-tile lies past N)
      // gets an offset past the descriptor's range, which reads nothing.  Those rows then take
      // exactly the statements of the plain epilogue below: bit-identical to a launch without delta.
      int sl[MT][4];
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) sl[m][r] = grp.dslot[min(m * 16 + (lane >> 4) * 4 + r, M - 1)];
      const __amdgpu_buffer_rsrc_t drs = dec_rsrc(grp.delta, (long)M * N * 4);
      float dv[MT][NTW][4];
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NTW; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = m * 16 + (lane >> 4) * 4 + r;
            const bool on = row < M && sl[m][r] >= 0 && sl[m][r] < grp.nslots && tile0 + t < (N >> 4);
            const uint32_t off = on ? (uint32_t)((row * N + (tile0 + t) * 16 + (lane & 15)) * 4) : 0x80000000u;
            dv[m][t][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(drs, off, 0, 0));
          }
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        float rs[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) rs[r] = rn_ss != nullptr ? s_inv[m * 16 + (lane >> 4) * 4 + r] : 1.f;
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
          const int tile = tile0 + t;
          if (tile >= (N >> 4)) continue;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = m * 16 + (lane >> 4) * 4 + r;
            float v = acc[m][t][r] * rs[r];
            if constexpr (F8) v *= wsc[t];
            if (row < M && sl[m][r] >= 0 && sl[m][r] < grp.nslots) v = dec_add_delta(v, dv[m][t][r]);
            dec_swiglu_store(Y, N >> 1, tile * 8 + (lane & 7), row, lane, v);
          }
        }
      }
      return;
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    float rs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) rs[r] = rn_ss != nullptr ? s_inv[m * 16 + (lane >> 4) * 4 + r] : 1.f;
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
      const int tile = tile0 + t;
      if (tile >= (N >> 4)) continue;  // the last workgroup of a grid that does not divide N
      if constexpr (EPI == DEC_SWIGLU8) {
        // n-tile rows [8 gate | 8 up] of features 8 tile .. 8 tile + 7: lane l (l & 8 == 0) holds
        // the gate of feature 8 tile + (l & 7), lane l ^ 8 the matching up
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[m][t][r] * rs[r];
          if constexpr (F8) v *= wsc[t];  // the [8 gate | 8 up] interleave permuted the scales with the rows
          dec_swiglu_store(Y, N >> 1, tile * 8 + (lane & 7), m * 16 + (lane >> 4) * 4 + r, lane, v);
        }
      } else {
        const int col = tile * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m * 16 + (lane >> 4) * 4 + r;
          if (row < M) {
            float v = acc[m][t][r] * rs[r];
            if constexpr (F8) v *= wsc[t];
            if constexpr (EPI == DEC_BF16)
              Y[(long)row * ldy + col] = f2bf(v);
            else
              partial[((long)(ex * gridDim.y + by) * M + row) * N + col] =
                  grp.rw != nullptr ? v * grp.rw[(long)row * grp.rw_ld + ex] : v;
          }
        }
      }
    }
  }
}


// Row-complete decode GEMM for a row-parallel projection feeding a residual add (the o projection
// of a TP=1 decode step): NO split-K slabs.  Each workgroup owns one 16-column n-tile for all M
// rows and the whole K; its 8 waves split K (one eighth each, the slices the split-K kernel's 8
// slabs had), stream their weight fragments AND their activation fragments straight into a
// register ring (the activations are L2-resident: every workgroup reads all of them), and reduce
// through LDS in slice order.  The epilogue then does what add_norm_partial_kernel did as its own
// launch over 8 MB of fp32 slabs:
//   resid <- bf16(resid + y)  (y summed slice by slice, in the slab kernel's order: bit-identical),
//   xw    <- bf16(resid * w)  fragment-packed as the next GEMM's A operand,
//   ss[row][tile] <- sum over the tile's 16 columns of resid^2 (the consumer's deferred RMSNorm
//                    sums N/16 partials per row).
// One launch and 16 MB of slab traffic fewer per layer; the price is the activation re-read from
// L2 (M x K bf16 per workgroup).
template <int MT, int DEPTH, int NKS>
__global__ __launch_bounds__(512, 1) void gemm_dec_rc_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                                             bf16_t* __restrict__ resid, const bf16_t* __restrict__ nw,
                                                             bf16_t* __restrict__ xw, float* __restrict__ ss_out,
                                                             int M, int N, int K) {
  constexpr int WAVES = 8;
  static_assert(NKS % DEPTH == 0, "the ring consumes whole DEPTH groups of k-steps");
  __shared__ __attribute__((aligned(16))) f32x4 red[WAVES][MT][64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int tile = blockIdx.x;
  const int ksteps = K >> 5;  // host: ksteps == 8 NKS
  constexpr int nks = NKS;     // k-steps per wave: compile-time, so every ring wait is a counted one
  const int kb = wave * nks;
  const u32x4* wp = reinterpret_cast<const u32x4*>(W) + ((long)tile * ksteps + kb) * 64 + lane;
  const u32x4* ap[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) ap[m] = reinterpret_cast<const u32x4*>(A) + ((long)m * ksteps + kb) * 64 + lane;
  u32x4 rw[DEPTH], ra[DEPTH][MT];
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    rw[d] = __builtin_nontemporal_load(wp + d * 64);
#pragma unroll
    for (int m = 0; m < MT; ++m) ra[d][m] = ap[m][d * 64];
  }
  f32x4 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k0 = 0; k0 < nks; k0 += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      const bf16x8 b = __builtin_bit_cast(bf16x8, rw[d]);
#pragma unroll
      for (int m = 0; m < MT; ++m)
        acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ra[d][m]), b, acc[m], 0, 0, 0);
      const int kn = k0 + d + DEPTH;
      if (kn < nks) {  // compile-time
        rw[d] = __builtin_nontemporal_load(wp + kn * 64);
#pragma unroll
        for (int m = 0; m < MT; ++m) ra[d][m] = ap[m][kn * 64];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) red[wave][m][lane] = acc[m];
  __syncthreads();
  if (wave >= MT) return;
  // wave m: m-tile m.  C layout: col = lane & 15, rows (lane >> 4) * 4 + r
  const int m = wave;
  const int col = tile * 16 + (lane & 15);
  const float wcol = bf2f(nw[col]);
  float ssr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = m * 16 + (lane >> 4) * 4 + r;
    const int rowc = min(row, M - 1);
    float h = bf2f(resid[(long)rowc * N + col]);
#pragma unroll
    for (int w = 0; w < WAVES; ++w) h += red[w][m][lane][r];  // slice order = the slab kernel's
    const bf16_t hb = f2bf(h);
    const float hv = bf2f(hb);
    ssr[r] = hv * hv;
    if (row < M) {
      resid[(long)row * N + col] = hb;
      xw[act_index(row, col, -(long)(N >> 5))] = f2bf(hv * wcol);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float v = ssr[r];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, kWave);  // the 16 columns of the row
    const int row = m * 16 + (lane >> 4) * 4 + r;
    if ((lane & 15) == 0 && row < M) ss_out[(long)row * (N >> 4) + tile] = v;
  }
}

}  // namespace k8sllm

using namespace k8sllm;

namespace {

struct DecLaunch {  // what every instantiation is launched with
  dim3 grid, blk;
  hipStream_t s;
  const bf16_t *A, *W;
  float* partial;
  bf16_t* Y;
  long ldy;
  int M, N, K, kchunk;
  const float* rn_ss;
  int rn_nc;
  float inv_d, rn_eps;
  DecGroup dg;
  const float* wscale;  // fp8 weights: one scale per packed weight row; mxfp4: the packed block scales (else null)
  int d4 = 0;           // mxfp4: the ring depth in k-steps (8 or 16)
  int flags = 0;        // kDecRows | kDecWt | kDecXcd (SLAB launches: dec_plan)
};

// Launches <mt m-tiles, form F> for 1 <= mt <= MT: the instantiations 1..MT of the form and no
// others (MT = 0: none).
// (D4: the mxfp4 ring depth, which replaces the form's own)
template <int F, bool RNW, int MT, int WF = DEC_W_BF16, int D4 = 0>
bool dec_launch(int mt, const DecLaunch& l) {
  if constexpr (MT == 0) {
    return false;
  } else {
    if (mt != MT) return dec_launch<F, RNW, MT - 1, WF, D4>(mt, l);
    constexpr DecForm f = kDecForms[F];
    constexpr int depth = WF == DEC_W_F4 ? D4 : f.depth;
    hipLaunchKernelGGL((gemm_dec_kernel<MT, f.ntw, f.waves, f.epi, depth, RNW, WF>), l.grid, l.blk, 0, l.s, l.A,
                       l.W, l.partial, l.Y, l.ldy, l.M, l.N, l.K, l.kchunk, l.rn_ss, l.rn_nc, l.inv_d, l.rn_eps, l.dg,
                       l.wscale, l.flags);
    return true;
  }
}

// The walk over kDecForms from row F on: false when no row is (epi, ntw, waves, depth) or the row
// has no instantiation for mt m-tiles (rnw: of the wide deferred-norm form; WF: of the fp8- or
// mxfp4-weight form - the rows of kDecF8Forms / kDecF4Forms, narrow norm only).
template <int WF = DEC_W_BF16, int F = 0>
bool dec_dispatch(int epi, int ntw, int waves, int depth, bool rnw, int mt, const DecLaunch& l) {
  if constexpr (F == kDecNForms) {
    return false;
  } else {
    constexpr DecForm f = kDecForms[F];
    if (epi != f.epi || ntw != f.ntw || waves != f.waves || depth != f.depth)
      return dec_dispatch<WF, F + 1>(epi, ntw, waves, depth, rnw, mt, l);
    if constexpr (WF == DEC_W_F8)
      return !rnw && dec_launch<F, false, dec_form_f8(F) ? f.max_mt : 0, DEC_W_F8>(mt, l);
    else if constexpr (WF == DEC_W_F4) {
      // ring depth 8 at 1..max_mt m-tiles, and 16 at one m-tile where kDecF4Forms says so (0: no row)
      constexpr int d1 = dec_form_f4_depth(F);
      if (rnw) return false;
      if (l.d4 == 16) return dec_launch<F, false, d1 >= 16 ? 1 : 0, DEC_W_F4, 16>(mt, l);
      return l.d4 == 8 && dec_launch<F, false, d1 >= 8 ? f.max_mt : 0, DEC_W_F4, 8>(mt, l);
    }
    else
      return rnw ? dec_launch<F, true, f.wide_norm ? kDecNarrowMaxMT : 0>(mt, l) : dec_launch<F, false, f.max_mt>(mt, l);
  }
}

}  // namespace

static_assert(kDecAChunk == kDecCH && kDecRnNarrow == 4 * kRnMax && kDecRnWide == 16 * kRnWide,
              "dec_plan (gemm_dec_forms.h) plans with the kernel's constants");

// THE launcher of gemm_dec_kernel, for every weight format (wf) and for dense (experts 0) and
// grouped (experts E >= 1: grid.z = expert) launches; what it accepts, the slicing and the grid are
// dec_plan's (gemm_dec_forms.h).
// W by wf: DEC_W_BF16 fragment-packed [N/16][K/32][64][8] (ops.pack_skinny), wscale unused;
// DEC_W_F8 e4m3 codes [N/16][K/64][64][16] (ops.pack_skinny_f8), wscale [N] fp32 powers of two in
// packed row order; DEC_W_F4 e2m1 codes [N/16][K/128][64][16], wscale the e8m0 block scales
// [N/16][K/128][16] dwords (ops.pack_skinny_f4).  For DEC_SWIGLU8 the weight rows are interleaved
// per 16-row n-tile as [8 gate | 8 up] (ops.interleave_gate_up8).  Grouped: one such weight (and
// scale tensor) per expert, w_eb / s_eb BYTES between them; a_es / y_es: elements between experts'
// A / SWIGLU8 outputs (a_es 0: A shared); SLAB slabs [E * splits][M][N], scaled by rw [M][rw_ld]
// where given.  ntw x waves n-tiles per workgroup - the last workgroup may hold fewer; depth:
// weight k-steps in flight per wave (mxfp4: f4_depth, see dec_plan).
// sw_rows / sw_wt / sw_xcd: dec_plan's switches for the SLAB epilogue and the split placement
// (-1 as shipped).
// delta / dslot / nslots: the pre-activation delta of a SWIGLU8 launch (DecGroup), or null.
// Returns 0, or dec_plan's negative code when the shape / configuration is not supported (the
// caller then uses gemm_skinny); -6: a delta this launch cannot take.
extern "C" int k8sllm_gemm_dec(const void* A, const void* W, const void* wscale, int wf, float* partial, void* Y,
                               long ldy, int M, int N, int K, int splits, int epi, int ntw, int waves, int depth,
                               int f4_depth, const float* rn_ss, int rn_nc, int rn_d, float rn_eps, int experts,
                               long a_es, long w_eb, long s_eb, long y_es, const float* rw, int rw_ld,
                               int sw_rows, int sw_wt, int sw_xcd, const float* delta, const int* dslot,
                               int nslots, hipStream_t s) {
  if (M <= 0) return 0;
  if (wf != DEC_W_BF16 && wscale == nullptr) return -1;
  // the pre-activation delta: the SWIGLU8 epilogue of a dense launch with the narrow deferred norm
  // (the wide one stands behind the row-complete o projection, which adapter steps do not take),
  // 16-byte aligned and under 2 GiB (32-bit buffer offsets)
  if (delta != nullptr &&
      (epi != DEC_SWIGLU8 || experts >= 1 || rw != nullptr || (rn_ss != nullptr && rn_nc > kDecRnNarrow) ||
       dslot == nullptr || nslots < 1 || reinterpret_cast<uintptr_t>(delta) % 16 || (long)M * N * 4 >= 0x7fffffffL))
    return -6;
  const DecPlan p = dec_plan(wf, M, N, K, splits, epi, ntw, waves, depth, f4_depth, experts, rw != nullptr,
                             rn_ss != nullptr ? rn_nc : 0, sw_rows, sw_wt, sw_xcd);
  if (p.err < 0) return p.err;
  // (16-byte stores need a 16-byte aligned workspace; any other keeps the 4-byte stores, same bits)
  const bool rows = p.rows && reinterpret_cast<uintptr_t>(partial) % 16 == 0;
  const int flags = (rows ? kDecRows : 0) | (rows && p.wt ? kDecWt : 0) | (p.xcd ? kDecXcd : 0);
  const DecLaunch l{dim3(p.gx, p.gy, p.gz), dim3(64 * waves), s, (const bf16_t*)A, (const bf16_t*)W, partial,
                    (bf16_t*)Y, ldy, M, N, K, p.kchunk, rn_ss, rn_nc, rn_d > 0 ? 1.f / (float)rn_d : 0.f, rn_eps,
                    DecGroup{a_es, y_es, w_eb, s_eb, rw, rw_ld, delta, delta != nullptr ? dslot : nullptr,
                             delta != nullptr ? nslots : 0},
                    wf == DEC_W_BF16 ? nullptr : (const float*)wscale,
                    p.d4, flags};
  bool ok = false;
  switch (wf) {
    case DEC_W_BF16: ok = dec_dispatch<DEC_W_BF16>(epi, ntw, waves, depth, p.rnw, p.mt, l); break;
    case DEC_W_F8: ok = dec_dispatch<DEC_W_F8>(epi, ntw, waves, depth, false, p.mt, l); break;
    case DEC_W_F4: ok = dec_dispatch<DEC_W_F4>(epi, ntw, waves, depth, false, p.mt, l); break;
  }
  if (!ok) return -5;
  return (int)hipGetLastError();
}

// The indices into kDecForms of the rows with fp8-weight instantiations (kDecF8Forms), at most
// cap of them into out; returns their count.
extern "C" int k8sllm_gemm_dec_f8_forms(int* out, int cap) {
  for (int i = 0; i < kDecNF8Forms && i < cap; ++i) out[i] = kDecF8Forms[i];
  return kDecNF8Forms;
}

// The rows of kDecForms with mxfp4-weight instantiations (kDecF4Forms) as two ints each (index
// into kDecForms, F4 ring depth at one m-tile), at most cap rows into out; returns the row count.
extern "C" int k8sllm_gemm_dec_f4_forms(int* out, int cap) {
  for (int i = 0; i < kDecNF4Forms && i < cap; ++i) {
    out[2 * i] = kDecF4Forms[i].form;
    out[2 * i + 1] = kDecF4Forms[i].depth;
  }
  return kDecNF4Forms;
}

// The rows of kDecForms as six ints each (epi, ntw, waves, depth, max_mt, wide_norm), at most cap
// rows into out; returns the row count.
extern "C" int k8sllm_gemm_dec_forms(int* out, int cap) {
  for (int i = 0; i < kDecNForms && i < cap; ++i) {
    const DecForm& f = kDecForms[i];
    const int row[6] = {f.epi, f.ntw, f.waves, f.depth, f.max_mt, f.wide_norm};
    for (int j = 0; j < 6; ++j) out[6 * i + j] = row[j];
  }
  return kDecNForms;
}


// Row-complete decode GEMM (gemm_dec_rc_kernel): A packed [ceil(M/16)][K/32][64][8], Wp packed
// [N/16][K/32][64][8]; resid [M][N] bf16 updated in place; xw packed [ceil(M/16)][N/32][64][8];
// ss [M][N/16] fp32.  Returns -1 for a shape the kernel does not tile.
extern "C" int k8sllm_gemm_dec_rc(const void* A, const void* Wp, void* resid, const void* nw, void* xw, float* ss,
                                  int M, int N, int K, hipStream_t s) {
  if (M <= 0) return 0;
  if (M > kDecNarrowMaxM || N % 32 || K % 32 || (K / 32) % 8) return -1;
  const int nks = K / 32 / 8;
  const int MT = (M + 15) / 16;
  const dim3 grid(N / 16), blk(512);
#define K8S_RC(MTV, DV, NK)                                                                                        \
  hipLaunchKernelGGL((gemm_dec_rc_kernel<MTV, DV, NK>), grid, blk, 0, s, (const bf16_t*)A, (const bf16_t*)Wp,    \
                     (bf16_t*)resid, (const bf16_t*)nw, (bf16_t*)xw, ss, M, N, K)
  if (nks == 16) {  // K = 4096: the o projection of Llama-3-8B / Mixtral at TP=1
    switch (MT) {
      case 1: K8S_RC(1, 8, 16); break;
      case 2: K8S_RC(2, 8, 16); break;
      case 3: K8S_RC(3, 8, 16); break;
      default: K8S_RC(4, 8, 16); break;
    }
  } else {  // (K = 14336, the down projection row-complete: bit-identical but 0.2-4.5 % slower per
            // decode step at 4-32 rows, profiles/r05/rc_down_*_ab.jsonl - removed)
    return -1;
  }
#undef K8S_RC
  return (int)hipGetLastError();
}
