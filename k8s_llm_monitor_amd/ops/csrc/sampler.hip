// Token sampler over logits[B][V].
//   temperature <= 0        -> greedy argmax (first index on ties, like torch.argmax)
//   temperature  > 0        -> Gumbel-max over logits/T  (exact sample from softmax(logits/T))
//   top_k > 0 / top_p < 1   -> the draw is over a kept set {x >= thr} (ops/reference.py sample_keep):
//                              top-k first (0 < k < V): thr = the k-th largest x / T, found exactly
//                              by bisecting its order-preserving integer image on the count;
//                              then top-p over the top-k survivors: the smallest prefix of their
//                              renormalised softmax, sorted descending, whose mass reaches p, found
//                              by bisecting the threshold on the mass.  Ties at either threshold
//                              are kept; no sort needed.
// Randomness is a counter hash of (seed, offset, row, index); `rng` lives in device memory so a
// hipGraph-captured decode step draws fresh numbers on every replay (the engine bumps offset).
//
// Decomposition: a decode batch has few rows (B <= 128 on the decode fast path; any B is taken -
// the part count comes from k8sllm_sample_parts(B, V)), and Gumbel-max over a 128K vocabulary is
// VALU-bound (hash + two logs per element), so one workgroup per row used 64 of 256 CUs and took
// 125 us at B = 64.  Rows are split into P parts: grid (B, P) of 1024-thread workgroups each
// produce a partial (value, index) argmax, and a one-wave kernel picks the winner per row.  Rows
// with top-k / top-p need a row-wide threshold; part 0 of such a row runs the whole-row bisection
// path and its answer is taken as is.  The per-element hash is 32-bit (two murmur3 finalisers of
// a per-row 64-bit key) - 64-bit multiplies are multi-instruction sequences on CDNA.
//
// Penalties (ops/reference.py apply_penalties): an optional device-resident state - a table
// [slots][tstride] of 16-bit entries (bit 15: the token is in the prompt, bits 0..14: how often it
// was generated, saturating) and (rep, 1/rep, presence, frequency) per slot.  A row with
// pslot[row] >= 0 reads every logit through `ldp<T, true>`, which penalises it before the
// pipeline above; the final kernel counts the drawn token in the row's slot, so a captured decode
// step keeps its own state the way it advances the RNG counter.  Without a table the kernels
// are the <T, false> instantiations: the plain loads.
//
// Guides (constrained decoding, guide.hip / ops.GuideState): a row with gslot[row] >= 0 whose slot
// holds a state >= 0 is guided - it reads every logit through `ldp<T, PEN, true>`, where a token
// whose bit in the state's mask row is clear reads as -inf (after penalisation, before everything
// else: greedy, the partial path and the whole-row top-k / top-p path all see the same row).  The
// 8 logits of a vector load take one mask byte.  The final kernel walks the drawn token's bytes
// from the slot's state and stores the new state, so a captured decode step advances the guide
// as it advances the RNG counter.  Without a guide state the kernels are the <T, PEN, false>
// instantiations, whose loads are those above.
#include <type_traits>

#include "common.h"
#include <stdlib.h>

namespace k8sllm {

constexpr int kST = 1024;

template <typename T>
__device__ __forceinline__ float ld(const T* p, long i);
template <>
__device__ __forceinline__ float ld<bf16_t>(const bf16_t* p, long i) { return bf2f(p[i]); }
template <>
__device__ __forceinline__ float ld<float>(const float* p, long i) { return p[i]; }

// one slot's penalty parameters (the slot's table row travels beside them as a plain pointer)
struct PenRow {
  float rep, inv_rep, presence, frequency;
};

constexpr uint32_t kPenSeen = 0x8000u, kPenCount = 0x7fffu;

// repetition penalty over prompt + output tokens, then frequency / presence over output tokens;
// each step rounded on its own (no contraction), like the fp32 reference
__device__ __forceinline__ float penalise(float x, uint32_t e, const PenRow& q) {
#pragma clang fp contract(off)
  if (e != 0u) x = x > 0.f ? x * q.inv_rep : x * q.rep;
  const uint32_t c = e & kPenCount;
  if (c == 0u) return x;
  const float fc = q.frequency * (float)c;
  return (x - fc) - q.presence;
}

// Logit i of a row as the sampler reads it: plain (PEN = false), or penalised by the row's table
// entries `cnt` (16-byte aligned) and parameters.
// GD: a token whose bit in the mask row `gm` (16-byte aligned) is clear reads as -inf.
template <typename T, bool PEN, bool GD>
__device__ __forceinline__ float ldp(const T* __restrict__ x, const uint16_t* __restrict__ cnt, const PenRow& q,
                                     const uint32_t* __restrict__ gm, int i) {
  float v = ld<T>(x, i);
  if constexpr (PEN) v = penalise(v, cnt[i], q);
  if constexpr (GD) {
    if (((gm[i >> 5] >> (i & 31)) & 1u) == 0u) v = -INFINITY;
  }
  return v;
}

// 8 logits from a 16-byte aligned bf16 address (and their 8 table entries, one 16-byte load; and
// their 8 mask bits, one byte: i is a multiple of 8)
template <bool PEN, bool GD>
__device__ __forceinline__ void ldp8(const bf16_t* __restrict__ x, const uint16_t* __restrict__ cnt,
                                     const PenRow& q, const uint32_t* __restrict__ gm, int i, float* v) {
  unpack8(*reinterpret_cast<const uint4*>(x + i), v);
  if constexpr (PEN) {
    const uint4 e = *reinterpret_cast<const uint4*>(cnt + i);
    const uint32_t w[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = penalise(v[2 * j], w[j] & 0xffffu, q);
      v[2 * j + 1] = penalise(v[2 * j + 1], w[j] >> 16, q);
    }
  }
  if constexpr (GD) {
    const uint32_t m = reinterpret_cast<const uint8_t*>(gm)[i >> 3];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (((m >> j) & 1u) == 0u) v[j] = -INFINITY;
  }
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ uint64_t row_key(const int64_t* rng, int row) {
  const uint64_t seed = rng ? (uint64_t)rng[0] : 0ull;
  const uint64_t off = rng ? (uint64_t)rng[1] : 0ull;
  return mix64(seed ^ mix64(off * 0x100000001b3ull + (uint64_t)row * 0x9e3779b97ull));
}

// Standard Gumbel noise -log(-log(u)).  u is drawn as 1 - w with w = (23-bit hash + 0.5) / 2^23,
// so w lies in [2^-24, 1 - 2^-24] and -log(u) = -log(1 - w) is taken by its series for small w:
// accurate and > 0 as u -> 1.
// (The earlier 24-bit u = (h + 0.5) / 2^24 rounded to exactly 1.0f for the top hash value, and the
// fast log of 1 is 0: a +inf noise that made an arbitrary token win - about once per two 64-row
// steps of a 128K vocabulary.)  Range: [-log(16.64), 16.64] = [-2.81, 16.64].
__device__ __forceinline__ float gumbel(uint64_t key, int i) {
  const uint32_t h = fmix32(fmix32((uint32_t)i * 0x9e3779b9u ^ (uint32_t)key) + (uint32_t)(key >> 32));
  const float w = ((float)(h >> 9) + 0.5f) * (1.0f / 8388608.0f);
  // -log(1 - w): the series w + w^2 / 2 below 2^-10 (relative error < 4e-7), the fast log above
  const float e = w < 0x1p-10f ? __builtin_fmaf(0.5f * w, w, w) : -__logf(1.f - w);
  return -__logf(e);
}

struct ArgMax {
  float v;
  int i;
};

__device__ __forceinline__ ArgMax better(ArgMax a, ArgMax b) {
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

__device__ __forceinline__ ArgMax block_argmax(ArgMax a, float* sv, int* si) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ArgMax b{__shfl_xor(a.v, o, 64), __shfl_xor(a.i, o, 64)};
    a = better(a, b);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sv[w] = a.v;
    si[w] = a.i;
  }
  __syncthreads();
  ArgMax r{sv[0], si[0]};
#pragma unroll
  for (int k = 1; k < kST / 64; ++k) r = better(r, ArgMax{sv[k], si[k]});
  __syncthreads();
  return r;
}

// Order-preserving image of an fp32 value: a < b as floats implies order_key(a) < order_key(b) as
// unsigned integers (-0 sorts just below +0); -inf -> 0x007fffff, +inf -> 0xff800000.
__device__ __forceinline__ uint32_t order_key(float f) {
  const int32_t b = __float_as_int(f);
  return (uint32_t)(b ^ ((b >> 31) | (int32_t)0x80000000));
}

__device__ __forceinline__ float order_key_inv(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// Whole-row path for rows with top-k / top-p (one workgroup); returns the token on every thread.
template <typename T, bool PEN, bool GD>
__device__ int sample_row_filtered(const T* __restrict__ x, const uint16_t* __restrict__ cnt, const PenRow& q,
                                   const uint32_t* __restrict__ gm, int V, float temp, int k, float p, uint64_t key,
                                   float* sv, int* si) {
  const int tid = threadIdx.x;
  const float itemp = 1.f / temp;
  float mx = -INFINITY, mn = INFINITY;
  for (int i = tid; i < V; i += kST) {
    const float v = ldp<T, PEN, GD>(x, cnt, q, gm, i) * itemp;
    mx = fmaxf(mx, v);
    mn = fminf(mn, v);
  }
  mx = block_max<kST>(mx, sv);
  mn = -block_max<kST>(-mn, sv);
  float thr = -INFINITY;
  if (k > 0 && k < V) {
    // the k-th largest value itself: the largest key t with count(key(v) >= t) >= k, built bit by
    // bit from the top (32 steps, exact for any range of the row, -inf included)
    uint32_t t = 0u;
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t cand = t | (1u << bit);
      float c = 0.f;  // V < 2^24: an exact count
      for (int i = tid; i < V; i += kST)
        c += (order_key(ldp<T, PEN, GD>(x, cnt, q, gm, i) * itemp) >= cand) ? 1.f : 0.f;
      c = block_sum<kST>(c, sv);
      if (c >= (float)k) t = cand;
    }
    thr = order_key_inv(t);
  }
  if (p < 1.f) {
    // mass over the top-k survivors only (thr = -inf without top-k: the whole row)
    float z = 0.f;
    for (int i = tid; i < V; i += kST) {
      const float v = ldp<T, PEN, GD>(x, cnt, q, gm, i) * itemp;
      z += (v >= thr) ? __expf(v - mx) : 0.f;
    }
    z = block_sum<kST>(z, sv);
    const float target = p * z;
    float lo = fmaxf(thr, fmaxf(mn, mx - 80.f)), hi = mx;  // invariant: mass(x >= lo) >= target
    for (int it = 0; it < 26; ++it) {
      const float mid = 0.5f * (lo + hi);
      float s = 0.f;
      for (int i = tid; i < V; i += kST) {
        const float v = ldp<T, PEN, GD>(x, cnt, q, gm, i) * itemp;
        s += (v >= mid) ? __expf(v - mx) : 0.f;
      }
      s = block_sum<kST>(s, sv);
      if (s >= target) lo = mid; else hi = mid;
    }
    thr = fmaxf(thr, lo);
  }
  ArgMax a{-INFINITY, 0x7fffffff};
  for (int i = tid; i < V; i += kST) {
    const float v = ldp<T, PEN, GD>(x, cnt, q, gm, i) * itemp;
    if (v >= thr) a = better(a, ArgMax{v + gumbel(key, i), i});
  }
  return block_argmax(a, sv, si).i;
}

__device__ __forceinline__ bool row_filtered(int V, float temp, int k, float p) {
  return temp > 0.f && ((k > 0 && k < V) || p < 1.f);
}

// part `part` of one row -> pv/pi[part] (pv, pi: the row's P partials)
template <typename T, bool PEN, bool GD>
__device__ __forceinline__ void sample_partial_row(float* __restrict__ pv, int* __restrict__ pi,
                                                   const T* __restrict__ x, const uint16_t* __restrict__ cnt,
                                                   const PenRow& q, const uint32_t* __restrict__ gm, long stride,
                                                   int V, int P, int part, int row, float temp, int k, float p,
                                                   const int64_t* __restrict__ rng, float* sv, int* si) {
  const int tid = threadIdx.x;
  if (row_filtered(V, temp, k, p)) {
    if (part != 0) return;
    const int tok = sample_row_filtered<T, PEN, GD>(x, cnt, q, gm, V, temp, k, p, row_key(rng, row), sv, si);
    if (tid == 0) pi[0] = tok;
    return;
  }
  // parts start on 8-element boundaries so that bf16 rows with an 8-aligned stride and a 16-byte
  // aligned base are read 16 B per lane (one load per 8 logits instead of eight dependent 2-byte
  // loads); any other row (a view that starts mid-vector) takes the scalar loop
  const int chunk = ((V + P - 1) / P + 7) & ~7;
  const int lo = min(V, part * chunk), hi = min(V, lo + chunk);
  const bool vec = std::is_same<T, bf16_t>::value && (stride & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(x + lo) & 15) == 0;
  const int hv = vec ? lo + ((hi - lo) & ~7) : lo;  // [lo, hv) in 8-element vectors, [hv, hi) scalar
  ArgMax a{-INFINITY, 0x7fffffff};
  const bool greedy = !(temp > 0.f);
  const float itemp = greedy ? 1.f : 1.f / temp;
  const uint64_t key = greedy ? 0ull : row_key(rng, row);
  if constexpr (std::is_same<T, bf16_t>::value) {
    for (int i = lo + tid * 8; i < hv; i += kST * 8) {
      float v[8];
      ldp8<PEN, GD>(x, cnt, q, gm, i, v);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        a = better(a, ArgMax{greedy ? v[j] : v[j] * itemp + gumbel(key, i + j), i + j});
    }
  }
  for (int i = hv + tid; i < hi; i += kST) {
    const float v = ldp<T, PEN, GD>(x, cnt, q, gm, i);
    a = better(a, ArgMax{greedy ? v : v * itemp + gumbel(key, i), i});
  }
  a = block_argmax(a, sv, si);
  if (tid == 0) {
    pv[part] = a.v;
    pi[part] = a.i;
  }
}

// grid (B, P): partial argmax of part `blockIdx.y` of row `blockIdx.x` -> pv/pi[row * P + part].
// PEN: rows with a slot (pslot[row] in [0, nslots)) are penalised - a row-uniform branch.
// GD: rows with a guide slot (gslot[row] in [0, gnslots)) whose state is a row of the guide arena
// ([0, grows)) read their logits through that row of gmask [grows][gW] - row-uniform too.
template <typename T, bool PEN, bool GD>
__global__ __launch_bounds__(kST) void sample_partial_kernel(float* __restrict__ pv, int* __restrict__ pi,
                                                             const T* __restrict__ logits, long stride, int V, int P,
                                                             const float* __restrict__ temps,
                                                             const int* __restrict__ top_k,
                                                             const float* __restrict__ top_p,
                                                             const int64_t* __restrict__ rng,
                                                             const int* __restrict__ pslot,
                                                             const uint16_t* __restrict__ table, long tstride,
                                                             const float4* __restrict__ pparams, int nslots,
                                                             const int* __restrict__ gslot,
                                                             const int* __restrict__ gstate, int gnslots,
                                                             const uint32_t* __restrict__ gmask, int gW, int grows) {
  __shared__ float sv[kST / 64];
  __shared__ int si[kST / 64];
  const int row = blockIdx.x, part = blockIdx.y;
  int slot = -1;
  if constexpr (PEN) slot = pslot[row];  // first, so the load is in flight with the row's parameters
  const uint32_t* gm = nullptr;
  if constexpr (GD) {
    const int gs = gslot[row];
    const int st = (unsigned)gs < (unsigned)gnslots ? gstate[gs] : -1;
    if ((unsigned)st < (unsigned)grows) gm = gmask + (long)st * gW;
  }
  const T* x = logits + (long)row * stride;
  const float temp = temps ? temps[row] : 0.f;
  const int k = top_k ? top_k[row] : 0;
  const float p = top_p ? top_p[row] : 1.f;
  pv += row * P;
  pi += row * P;
  if constexpr (PEN) {
    if (slot >= 0 && slot < nslots) {
      const float4 q = pparams[slot];
      if constexpr (GD) {
        if (gm != nullptr) {
          sample_partial_row<T, true, true>(pv, pi, x, table + (long)slot * tstride, PenRow{q.x, q.y, q.z, q.w}, gm,
                                            stride, V, P, part, row, temp, k, p, rng, sv, si);
          return;
        }
      }
      sample_partial_row<T, true, false>(pv, pi, x, table + (long)slot * tstride, PenRow{q.x, q.y, q.z, q.w}, nullptr,
                                         stride, V, P, part, row, temp, k, p, rng, sv, si);
      return;
    }
  }
  if constexpr (GD) {
    if (gm != nullptr) {
      sample_partial_row<T, false, true>(pv, pi, x, nullptr, PenRow{}, gm, stride, V, P, part, row, temp, k, p, rng,
                                         sv, si);
      return;
    }
  }
  sample_partial_row<T, false, false>(pv, pi, x, nullptr, PenRow{}, nullptr, stride, V, P, part, row, temp, k, p, rng,
                                      sv, si);
}

// one thread per row: the best of the P partials (or part 0's answer for a filtered row)
__global__ __launch_bounds__(64) void sample_final_kernel(int* __restrict__ out, const float* __restrict__ pv,
                                                          const int* __restrict__ pi, int B, int V, int P,
                                                          const float* __restrict__ temps,
                                                          const int* __restrict__ top_k,
                                                          const float* __restrict__ top_p,
                                                          int64_t* __restrict__ rng_advance,
                                                          const int* __restrict__ pslot,
                                                          uint16_t* __restrict__ table, long tstride, int nslots,
                                                          const int* __restrict__ gslot, int* __restrict__ gstate,
                                                          int gnslots, const int* __restrict__ gtrans, int grows,
                                                          const int* __restrict__ tok_off,
                                                          const uint8_t* __restrict__ blob,
                                                          const int* __restrict__ eos_ids, int n_eos) {
  const int row = blockIdx.x * 64 + threadIdx.x;
  // the partial kernel has drawn this step's numbers: advance the counter for the next step here
  // (one lane, a vector store) instead of a separate `rng[1] += 1` launch after every sample
  if (rng_advance != nullptr && row == 0) rng_advance[1] = rng_advance[1] + 1;
  if (row >= B) return;
  const int slot = table != nullptr ? pslot[row] : -1;  // issued first: in flight while the partials are read
  const int gs = gstate != nullptr ? gslot[row] : -1;
  const float temp = temps ? temps[row] : 0.f;
  const int k = top_k ? top_k[row] : 0;
  const float p = top_p ? top_p[row] : 1.f;
  int tok;
  if (row_filtered(V, temp, k, p)) {
    tok = pi[row * P];
  } else {
    ArgMax a{pv[row * P], pi[row * P]};
    for (int j = 1; j < P; ++j) a = better(a, ArgMax{pv[row * P + j], pi[row * P + j]});
    tok = a.i;
  }
  out[row] = tok;
  // count the drawn token in the row's slot (live rows hold distinct slots: a plain
  // read-modify-write); a row of NaNs draws no token in [0, V) and counts nothing
  if (slot >= 0 && slot < nslots && (unsigned)tok < (unsigned)V) {
    uint16_t* e = table + (long)slot * tstride + tok;
    const uint32_t c = *e;
    if ((c & kPenCount) != kPenCount) *e = (uint16_t)(c + 1u);
  }
  // walk the drawn token's bytes from the row's guide state (live rows hold distinct slots); an
  // eos token, a token outside [0, V), a token without bytes and a walk that would die leave it
  if ((unsigned)gs < (unsigned)gnslots && (unsigned)tok < (unsigned)V) {
    int st = gstate[gs];
    if ((unsigned)st >= (unsigned)grows) return;
    for (int e = 0; e < n_eos; ++e)
      if (eos_ids[e] == tok) return;
    const int b0 = tok_off[tok], b1 = tok_off[tok + 1];
    for (int j = b0; j < b1 && (unsigned)st < (unsigned)grows; ++j) st = gtrans[(long)st * 256 + blob[j]];
    if (b1 > b0 && (unsigned)st < (unsigned)grows) gstate[gs] = st;
  }
}

// One workgroup: clear a slot's table row, set its parameters, then mark ids[0, n_prompt) as seen
// and count ids[n_prompt, n_prompt + n_out) (repeated ids add up; ids outside [0, V) are skipped).
__global__ __launch_bounds__(kST) void penalty_reset_kernel(uint16_t* __restrict__ trow, int V, int tstride,
                                                            const int* __restrict__ ids, int n_prompt, int n_out,
                                                            float4* __restrict__ params, float4 q) {
  const int tid = threadIdx.x;
  uint4* r4 = reinterpret_cast<uint4*>(trow);
  for (int i = tid; i < tstride / 8; i += kST) r4[i] = make_uint4(0u, 0u, 0u, 0u);
  if (tid == 0) *params = q;
  __syncthreads();
  for (int j = tid; j < n_prompt; j += kST) {
    const int id = ids[j];
    if ((unsigned)id < (unsigned)V) trow[id] = (uint16_t)kPenSeen;  // the same value from every writer
  }
  __syncthreads();
  // 16-bit entries, 32-bit atomics: a saturating increment of one half of the aligned word
  uint32_t* w32 = reinterpret_cast<uint32_t*>(trow);
  for (int j = tid; j < n_out; j += kST) {
    const int id = ids[n_prompt + j];
    if ((unsigned)id >= (unsigned)V) continue;
    uint32_t* w = w32 + (id >> 1);
    const int sh = (id & 1) * 16;
    uint32_t old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (((old >> sh) & kPenCount) != kPenCount) {
      const uint32_t seen = atomicCAS(w, old, old + (1u << sh));
      if (seen == old) break;
      old = seen;
    }
  }
}

}  // namespace k8sllm

using namespace k8sllm;

extern "C" int k8sllm_sample_parts(long B, int V) {
  // ~2 workgroups per CU in total, at least 8K vocabulary entries per part
  long p = (512 + B - 1) / B;
  p = p < 1 ? 1 : p;
  const long pmax = V / 8192 > 1 ? V / 8192 : 1;
  return (int)(p < pmax ? p : pmax);
}

// pv/pi: workspace of at least B * k8sllm_sample_parts(B, V) entries.  Penalties: `table` (null =
// none) [nslots][tstride] with tstride a multiple of 8 and a 16-byte aligned base, `pparams`
// [nslots] x (rep, 1/rep, presence, frequency), `pslot` [B] (-1 = the row has no penalties).
// Guides: `gmask` (null = none) [grows][gW] with gW a multiple of 4 words covering V and a 16-byte
// aligned base, `gtrans` [grows][256] absolute rows, `gstate` [gnslots] (-1 = unguided), `gslot` [B]
// (-1 = the row has no guide), the vocabulary as CSR (`tok_off` [V + 1], `blob`) and the eos ids.
extern "C" int k8sllm_sample_guided(int* out, const void* logits, int is_fp32, long B, long stride, int V,
                                    const float* temps, const int* top_k, const float* top_p, const int64_t* rng,
                                    float* pv, int* pi, int advance, const int* pslot, void* table, long tstride,
                                    const float* pparams, int nslots, const int* gslot, int* gstate, int gnslots,
                                    const void* gmask, int gW, const int* gtrans, int grows, const int* tok_off,
                                    const void* blob, const int* eos_ids, int n_eos, hipStream_t s) {
  if (B <= 0) return 0;
  if (table != nullptr && (pslot == nullptr || pparams == nullptr || tstride < V || (tstride & 7) != 0 ||
                           (reinterpret_cast<uintptr_t>(table) & 15) != 0 ||
                           (reinterpret_cast<uintptr_t>(pparams) & 15) != 0))
    return (int)hipErrorInvalidValue;
  if (gmask != nullptr && (gslot == nullptr || gstate == nullptr || gtrans == nullptr || tok_off == nullptr ||
                           blob == nullptr || gnslots <= 0 || grows <= 0 || (gW & 3) != 0 || (long)gW * 32 < V ||
                           n_eos < 0 || (n_eos > 0 && eos_ids == nullptr) ||
                           (reinterpret_cast<uintptr_t>(gmask) & 15) != 0))
    return (int)hipErrorInvalidValue;
  const int P = k8sllm_sample_parts(B, V);
  dim3 grid((unsigned)B, P);
  uint16_t* tb = (uint16_t*)table;
  const float4* pp = (const float4*)pparams;
  const uint32_t* gm = (const uint32_t*)gmask;
#define K8SLLM_SAMPLE_PARTIAL(T, PEN, GD)                                                                       \
  hipLaunchKernelGGL((sample_partial_kernel<T, PEN, GD>), grid, dim3(kST), 0, s, pv, pi, (const T*)logits, stride, V, \
                     P, temps, top_k, top_p, rng, pslot, tb, tstride, pp, nslots, gslot, gstate, gnslots, gm, gW, grows)
#define K8SLLM_SAMPLE_T(T)                                                                        \
  do {                                                                                            \
    if (gm) {                                                                                     \
      if (tb) K8SLLM_SAMPLE_PARTIAL(T, true, true); else K8SLLM_SAMPLE_PARTIAL(T, false, true);   \
    } else {                                                                                      \
      if (tb) K8SLLM_SAMPLE_PARTIAL(T, true, false); else K8SLLM_SAMPLE_PARTIAL(T, false, false); \
    }                                                                                             \
  } while (0)
  if (is_fp32) K8SLLM_SAMPLE_T(float); else K8SLLM_SAMPLE_T(bf16_t);
#undef K8SLLM_SAMPLE_T
#undef K8SLLM_SAMPLE_PARTIAL
  hipLaunchKernelGGL(sample_final_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, out, pv, pi, (int)B, V, P,
                     temps, top_k, top_p, advance && rng ? const_cast<int64_t*>(rng) : nullptr, pslot, tb, tstride,
                     nslots, gslot, gm ? gstate : nullptr, gnslots, gtrans, grows, tok_off, (const uint8_t*)blob,
                     eos_ids, n_eos);
  return (int)hipGetLastError();
}

extern "C" int k8sllm_sample_pen(int* out, const void* logits, int is_fp32, long B, long stride, int V,
                                 const float* temps, const int* top_k, const float* top_p, const int64_t* rng,
                                 float* pv, int* pi, int advance, const int* pslot, void* table, long tstride,
                                 const float* pparams, int nslots, hipStream_t s) {
  return k8sllm_sample_guided(out, logits, is_fp32, B, stride, V, temps, top_k, top_p, rng, pv, pi, advance, pslot,
                              table, tstride, pparams, nslots, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr,
                              nullptr, nullptr, 0, s);
}

extern "C" int k8sllm_sample(int* out, const void* logits, int is_fp32, long B, long stride, int V,
                             const float* temps, const int* top_k, const float* top_p, const int64_t* rng,
                             float* pv, int* pi, int advance, hipStream_t s) {
  return k8sllm_sample_pen(out, logits, is_fp32, B, stride, V, temps, top_k, top_p, rng, pv, pi, advance, nullptr,
                           nullptr, 0, nullptr, 0, s);
}

// ids: n_prompt prompt ids followed by n_out output ids (device memory); no host sync
extern "C" int k8sllm_penalty_reset(void* table, long tstride, int V, int nslots, int slot, const int* ids,
                                    int n_prompt, int n_out, float* pparams, float rep, float inv_rep, float presence,
                                    float frequency, hipStream_t s) {
  if (slot < 0 || slot >= nslots || tstride < V || (tstride & 7) != 0 || n_prompt < 0 || n_out < 0 ||
      (reinterpret_cast<uintptr_t>(table) & 15) != 0 || (reinterpret_cast<uintptr_t>(pparams) & 15) != 0)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(penalty_reset_kernel, dim3(1), dim3(kST), 0, s, (uint16_t*)table + (long)slot * tstride, V,
                     (int)tstride, ids, n_prompt, n_out, (float4*)pparams + slot,
                     make_float4(rep, inv_rep, presence, frequency));
  return (int)hipGetLastError();
}
