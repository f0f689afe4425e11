// Per-request low-rank adapters (LoRA) on the serving path (ops.lora_slab / ops.lora_add,
// reference: ops/reference.py lora_delta):
//
//   delta[row, :] = scaling[s] * B[s] (A[s] x[row]),   s = slot[row] >= 0;   slot[row] < 0: no adapter
//
// over a device arena A [slots][R][K] bf16, B [slots][N][R] bf16, scaling [slots] fp32 (R = the
// projection's rank capacity, smaller ranks zero-padded).  Two launches:
//
//   lora_shrink_kernel   t_part[sp][row][0..R) = A[s] . x[row] over K slice sp   (bf16 MFMA, fp32 out)
//   lora_expand_kernel   t = sum_sp t_part[sp] in index order (fp32, never rounded to bf16), then
//                        delta = scaling[s] * B[s] . t on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32)
//
// Rows of one 16-row tile may name different adapters.  Both kernels loop over the ADAPTERS present
// among a workgroup's rows, not over rows: for adapter s the activation fragment of every row that
// does not name s is replaced by zeros (a select, so padding rows may hold anything), and all
// adapters accumulate into the one accumulator tile - a row only ever receives products of its own
// adapter plus exact zeros.  Each A / B element is thus read once per (adapter present, workgroup).
//
// shrink: grid (R/16, S, ceil(M/128)), one wave per workgroup: r-tile x K slice x up to 8 m-tiles
// (the A fragment of a k-step is loaded once and used by every m-tile).  x is the fragment-packed
// decode operand [ceil(M/16)][K/32][64][8] - already the MFMA A fragment - or row-major [M][K].
// Optional deferred RMSNorm: t *= rsqrt(sum(ss_part[row]) / K + eps) (the packed operand of
// add_norm_partial is residual * norm_w without the 1/rms).  S = k8sllm_lora_shrink_plan(K).
// expand: grid (ceil(N/64), ceil(M/64)), 4 waves: the workgroup sums its 64 rows' partials into LDS
// once, then each wave owns one 16-column n-tile.  Output: an fp32 slab [M][N] (rows without an
// adapter are written as exact zeros - the slab's consumers sum it), or a bf16 add in place
// (y = bf16(float(y) + delta); rows without an adapter are not touched).
// No atomics, every sum in a fixed order: the same input gives the same bits on every launch.
#include "common.h"

namespace k8sllm {
namespace {

constexpr int kShrinkMT = 8;   // m-tiles of a shrink workgroup (128 rows)
constexpr int kShrinkU = 4;    // k-steps whose loads a shrink wave keeps in flight together (written out below)
constexpr int kExpandMT = 4;   // m-tiles of an expand workgroup (64 rows)
constexpr int kExpandPad = 8;  // floats of padding per LDS row of t: 16 rows spread over the banks

// slot of a row as the kernels use it: -1 for "no adapter", for rows past M and for anything
// outside the arena (an out-of-range slot must never become an address)
__device__ __forceinline__ int row_slot(const int* __restrict__ slot, long row, long M, int nslots) {
  if (row >= M) return -1;
  const int s = slot[row];
  return (s >= 0 && s < nslots) ? s : -1;
}

template <bool PACKED>
__global__ __launch_bounds__(64) void lora_shrink_kernel(const bf16_t* __restrict__ x, long xstride,
                                                         const bf16_t* __restrict__ A, const int* __restrict__ slot,
                                                         const float* __restrict__ ss_part, int ss_cols, float eps,
                                                         float* __restrict__ t_part, long M, int R, int K, int nslots,
                                                         int ksteps) {
  const int lane = threadIdx.x;
  const int r = lane & 15, q = lane >> 4;
  const int rt = blockIdx.x, sp = blockIdx.y;
  const long m0 = (long)blockIdx.z * (16 * kShrinkMT);
  __shared__ float s_scale[16 * kShrinkMT];
#pragma unroll
  for (int i = lane; i < 16 * kShrinkMT; i += 64) {
    float sc = 1.f;
    if (ss_part != nullptr && m0 + i < M) {
      float ss = 0.f;
      for (int c = 0; c < ss_cols; ++c) ss += ss_part[(m0 + i) * ss_cols + c];
      sc = rsqrtf(ss / (float)K + eps);
    }
    s_scale[i] = sc;
  }
  int sl[kShrinkMT];
#pragma unroll
  for (int mt = 0; mt < kShrinkMT; ++mt) sl[mt] = row_slot(slot, m0 + 16 * mt + r, M, nslots);
  __syncthreads();

  f32x4 acc[kShrinkMT];
#pragma unroll
  for (int mt = 0; mt < kShrinkMT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = K / 32;
  const int ks0 = sp * ksteps, ks1 = min(nk, ks0 + ksteps);
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  for (int s = 0; s < nslots; ++s) {
    unsigned tiles = 0;  // m-tiles with a row of adapter s (wave-uniform)
#pragma unroll
    for (int mt = 0; mt < kShrinkMT; ++mt) tiles |= (__ballot(sl[mt] == s) != 0ull ? 1u : 0u) << mt;
    if (tiles == 0) continue;
    const bf16_t* As = A + ((size_t)s * R + 16 * rt + r) * K + 8 * q;
    // kShrinkU k-steps per round, every load of a round issued before its first MFMA: one load
    // latency per round instead of one per k-step (the k order of the sums is unchanged)
    for (int ks = ks0; ks < ks1; ks += kShrinkU) {
      const int nu = min(kShrinkU, ks1 - ks);  // wave-uniform
      uint4 b0 = zero, b1 = zero, b2 = zero, b3 = zero;
      b0 = *reinterpret_cast<const uint4*>(As + 32 * ks);
      if (nu > 1) b1 = *reinterpret_cast<const uint4*>(As + 32 * (ks + 1));
      if (nu > 2) b2 = *reinterpret_cast<const uint4*>(As + 32 * (ks + 2));
      if (nu > 3) b3 = *reinterpret_cast<const uint4*>(As + 32 * (ks + 3));
#pragma unroll
      for (int mt = 0; mt < kShrinkMT; ++mt) {
        if (tiles & (1u << mt)) {  // wave-uniform
          uint4 a0 = zero, a1 = zero, a2 = zero, a3 = zero;
          if (sl[mt] == s) {  // implies row < M
            const bf16_t* xp = x + (PACKED ? ((((size_t)blockIdx.z * kShrinkMT + mt) * nk + ks) * 64 + lane) * 8
                                           : (size_t)(m0 + 16 * mt + r) * xstride + 32 * ks + 8 * q);
            const size_t step = PACKED ? 64 * 8 : 32;  // elements from one k-step to the next
            a0 = *reinterpret_cast<const uint4*>(xp);
            if (nu > 1) a1 = *reinterpret_cast<const uint4*>(xp + step);
            if (nu > 2) a2 = *reinterpret_cast<const uint4*>(xp + 2 * step);
            if (nu > 3) a3 = *reinterpret_cast<const uint4*>(xp + 3 * step);
          }
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a0),
                                                            __builtin_bit_cast(bf16x8, b0), acc[mt], 0, 0, 0);
          if (nu > 1)
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a1),
                                                              __builtin_bit_cast(bf16x8, b1), acc[mt], 0, 0, 0);
          if (nu > 2)
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a2),
                                                              __builtin_bit_cast(bf16x8, b2), acc[mt], 0, 0, 0);
          if (nu > 3)
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a3),
                                                              __builtin_bit_cast(bf16x8, b3), acc[mt], 0, 0, 0);
        }
      }
    }
  }
  // C layout: column (r index) = lane & 15, row = 4 * (lane >> 4) + reg
#pragma unroll
  for (int mt = 0; mt < kShrinkMT; ++mt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int rl = 16 * mt + 4 * q + g;
      if (m0 + rl < M) t_part[((size_t)sp * M + m0 + rl) * R + 16 * rt + r] = acc[mt][g] * s_scale[rl];
    }
}

template <bool SLAB>
__global__ __launch_bounds__(256) void lora_expand_kernel(const float* __restrict__ t_part, int S,
                                                          const bf16_t* __restrict__ B,
                                                          const float* __restrict__ scaling,
                                                          const int* __restrict__ slot, float* __restrict__ slab,
                                                          bf16_t* __restrict__ y, long ystride, long M, int N, int R,
                                                          int nslots) {
  extern __shared__ __attribute__((aligned(16))) float s_t[];  // [64][R + kExpandPad]
  __shared__ int s_slot[16 * kExpandMT];
  __shared__ float s_scal[16 * kExpandMT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const long m0 = (long)blockIdx.y * (16 * kExpandMT);
  const int ld = R + kExpandPad;
  if (tid < 16 * kExpandMT) {
    const int s = row_slot(slot, m0 + tid, M, nslots);
    s_slot[tid] = s;
    s_scal[tid] = s >= 0 ? scaling[s] : 0.f;
  }
  // t = the S partials summed in index order, fp32; zeros for rows without an adapter
  const int r4 = R / 4;
  for (int i = tid; i < 16 * kExpandMT * r4; i += 256) {
    const int rl = i / r4, c = (i - rl * r4) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row_slot(slot, m0 + rl, M, nslots) >= 0) {
      for (int sp = 0; sp < S; ++sp) {
        const float4 p = *reinterpret_cast<const float4*>(t_part + ((size_t)sp * M + m0 + rl) * R + c);
        v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
      }
    }
    *reinterpret_cast<float4*>(s_t + rl * ld + c) = v;
  }
  __syncthreads();
  const int nt = blockIdx.x * 4 + w;
  if (16 * nt >= N) return;  // no barrier below

  int sl[kExpandMT];
#pragma unroll
  for (int mt = 0; mt < kExpandMT; ++mt) sl[mt] = s_slot[16 * mt + r];
  f32x4 acc[kExpandMT];
#pragma unroll
  for (int mt = 0; mt < kExpandMT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < nslots; ++s) {
    unsigned tiles = 0;
#pragma unroll
    for (int mt = 0; mt < kExpandMT; ++mt) tiles |= (__ballot(sl[mt] == s) != 0ull ? 1u : 0u) << mt;
    if (tiles == 0) continue;
    const bf16_t* Bs = B + ((size_t)s * N + 16 * nt + r) * R + 8 * q;
    for (int r0 = 0; r0 < R; r0 += 32) {
      // lane (n = r, k group q) holds B[n][r0 + 8 q + j], j = 0..7: MFMA sub-step j sums the four
      // rank indices r0 + 8 q' + j, q' = 0..3 - the t operand below uses the same assignment
      float bf[8];
      unpack8(*reinterpret_cast<const uint4*>(Bs + r0), bf);
#pragma unroll
      for (int mt = 0; mt < kExpandMT; ++mt) {
        if (!(tiles & (1u << mt))) continue;  // wave-uniform
        const float* tp = s_t + (16 * mt + r) * ld + r0 + 8 * q;
        const float4 t0 = *reinterpret_cast<const float4*>(tp);
        const float4 t1 = *reinterpret_cast<const float4*>(tp + 4);
        const bool on = sl[mt] == s;
        const float tv[8] = {on ? t0.x : 0.f, on ? t0.y : 0.f, on ? t0.z : 0.f, on ? t0.w : 0.f,
                             on ? t1.x : 0.f, on ? t1.y : 0.f, on ? t1.z : 0.f, on ? t1.w : 0.f};
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(tv[j], bf[j], acc[mt], 0, 0, 0);
      }
    }
  }
  const int col = 16 * nt + r;
#pragma unroll
  for (int mt = 0; mt < kExpandMT; ++mt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int rl = 16 * mt + 4 * q + g;
      const long row = m0 + rl;
      if (row >= M) continue;
      const bool has = s_slot[rl] >= 0;
      const float d = s_scal[rl] * acc[mt][g];
      if constexpr (SLAB) {
        slab[(size_t)row * N + col] = has ? d : 0.f;
      } else if (has) {
        bf16_t* p = y + (size_t)row * ystride + col;
        *p = f2bf(bf2f(*p) + d);
      }
    }
}

}  // namespace
}  // namespace k8sllm

using namespace k8sllm;

extern "C" {

// K slices of a shrink launch (t_part [S][M][R]): about 512 deep, at most 16, whole 32-deep k-steps
int k8sllm_lora_shrink_plan(int K) {
  const int nk = K / 32;
  if (K <= 0 || K % 32) return 0;
  int s0 = K / 512;
  s0 = s0 < 1 ? 1 : (s0 > 16 ? 16 : s0);
  const int per = (nk + s0 - 1) / s0;
  return (nk + per - 1) / per;
}

// returns a hipError_t, or -1 for a shape the kernels do not take
int k8sllm_lora_shrink(const void* x, int packed, long xstride, const void* A, const int* slot, const float* ss_part,
                       int ss_cols, float eps, float* t_part, long M, int R, int K, int nslots, hipStream_t st) {
  const int S = k8sllm_lora_shrink_plan(K);
  if (S <= 0 || R <= 0 || R % 16 || M <= 0 || nslots <= 0) return -1;
  if (!packed && xstride % 8) return -1;
  const long mg = (M + 16 * kShrinkMT - 1) / (16 * kShrinkMT);
  if (mg > 65535) return -1;
  const int nk = K / 32;
  const int per = (nk + S - 1) / S;
  const dim3 grid(R / 16, S, (unsigned)mg);
  const bf16_t* xp = (const bf16_t*)x;
  const bf16_t* Ap = (const bf16_t*)A;
  if (packed)
    hipLaunchKernelGGL(lora_shrink_kernel<true>, grid, dim3(64), 0, st, xp, xstride, Ap, slot, ss_part, ss_cols, eps,
                       t_part, M, R, K, nslots, per);
  else
    hipLaunchKernelGGL(lora_shrink_kernel<false>, grid, dim3(64), 0, st, xp, xstride, Ap, slot, ss_part, ss_cols, eps,
                       t_part, M, R, K, nslots, per);
  return (int)hipGetLastError();
}

int k8sllm_lora_expand(const float* t_part, int S, const void* B, const float* scaling, const int* slot, float* slab,
                       void* y, long ystride, long M, int N, int R, int nslots, hipStream_t st) {
  if (S <= 0 || R <= 0 || R % 32 || N <= 0 || N % 16 || M <= 0 || nslots <= 0) return -1;
  const size_t lds = (size_t)16 * kExpandMT * (R + kExpandPad) * sizeof(float);
  if (lds > 60 * 1024) return -1;
  const long mg = (M + 16 * kExpandMT - 1) / (16 * kExpandMT);
  if (mg > 65535 || (slab == nullptr) == (y == nullptr)) return -1;
  const dim3 grid((N + 63) / 64, (unsigned)mg);
  const bf16_t* Bp = (const bf16_t*)B;
  if (slab != nullptr)
    hipLaunchKernelGGL(lora_expand_kernel<true>, grid, dim3(256), lds, st, t_part, S, Bp, scaling, slot, slab,
                       (bf16_t*)nullptr, 0L, M, N, R, nslots);
  else
    hipLaunchKernelGGL(lora_expand_kernel<false>, grid, dim3(256), lds, st, t_part, S, Bp, scaling, slot,
                       (float*)nullptr, (bf16_t*)y, ystride, M, N, R, nslots);
  return (int)hipGetLastError();
}

}  // extern "C"
