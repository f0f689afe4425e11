// Token log-probabilities beside the sampler (ops/reference.py token_logprobs).
//   lp(t)  = x[t] - lse,  lse = m + log(sum_i exp(x[i] - m)),  m = max_i x[i], over the logits as
//            the LM head wrote them (bf16 or fp32, read as fp32): the model's distribution, before
//            penalties, temperature and top-k / top-p;
//   top n  = the n largest logits of the row in the order (value descending, index ascending), each
//            with its x[id] - lse (0 <= n <= kLpMaxTop).
// want[row] < 0: the row did not ask and nothing of it is read or written; 0: lp(tok) only;
// 1..kLpMaxTop: plus that many alternatives.
//
// Decomposition: the sampler's.  Grid (B, P) of 1024-thread workgroups with P =
// k8sllm_sample_parts(B, V) and the same 8-aligned part boundaries (sampler.hip
// sample_partial_row), so a row's logits are read the same way: 16 bytes per lane from a bf16 row
// with an 8-aligned stride and a 16-byte aligned part base, the scalar loop otherwise.  Each part
// writes (max, sum exp(x - max)) and its own top want[row] candidates, sorted; a one-wave kernel
// per row merges the P pairs in part order, merges the P sorted lists and reads x[tok[row]].
//
// Selection is exact under ties and keeps nothing in scratch: every thread holds the best of its
// own elements that lies strictly after the previous winner in (value desc, index asc) order; a
// round is one workgroup argmax, and only the thread that owned the winner scans its elements
// again (the part is a few tens of KiB and L2-resident).  No float atomics: every sum has a fixed
// order, so the same input gives the same bits on every launch.
#include <type_traits>

#include "common.h"

namespace k8sllm {
namespace {

constexpr int kLT = 1024;        // threads of a partial workgroup
constexpr int kLpMaxTop = 20;    // OpenAI's top_logprobs limit
constexpr int kLpWidth = 1 + 2 * kLpMaxTop;
constexpr int kNone = 0x7fffffff;  // index of "no element"

struct Cand {
  float v;
  int i;
};

// a before b in (value descending, index ascending) order
__device__ __forceinline__ bool before(Cand a, Cand b) { return a.v > b.v || (a.v == b.v && a.i < b.i); }

__device__ __forceinline__ Cand best(Cand a, Cand b) { return before(b, a) ? b : a; }

__device__ __forceinline__ Cand wave_best(Cand a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = best(a, Cand{__shfl_xor(a.v, o, 64), __shfl_xor(a.i, o, 64)});
  return a;
}

__device__ __forceinline__ Cand block_best(Cand a, float* sv, int* si) {
  a = wave_best(a);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sv[w] = a.v;
    si[w] = a.i;
  }
  __syncthreads();
  Cand r{sv[0], si[0]};
#pragma unroll
  for (int k = 1; k < kLT / 64; ++k) r = best(r, Cand{sv[k], si[k]});
  __syncthreads();
  return r;
}

template <typename T>
__device__ __forceinline__ float ldx(const T* p, long i);
template <>
__device__ __forceinline__ float ldx<bf16_t>(const bf16_t* p, long i) { return bf2f(p[i]); }
template <>
__device__ __forceinline__ float ldx<float>(const float* p, long i) { return p[i]; }

// This thread's elements of [lo, hi) - [lo, hv) as 8-element vectors, [hv, hi) one by one - as
// f(value, index)
template <typename T, typename F>
__device__ __forceinline__ void for_mine(const T* __restrict__ x, int lo, int hv, int hi, F f) {
  const int tid = threadIdx.x;
  if constexpr (std::is_same<T, bf16_t>::value) {
    for (int i = lo + tid * 8; i < hv; i += kLT * 8) {
      float v[8];
      unpack8(*reinterpret_cast<const uint4*>(x + i), v);
#pragma unroll
      for (int j = 0; j < 8; ++j) f(v[j], i + j);
    }
  }
  for (int i = hv + tid; i < hi; i += kLT) f(ldx<T>(x, i), i);
}

// the best of this thread's elements strictly after `prev` ({-inf, kNone}: none; a NaN is never one)
template <typename T>
__device__ __forceinline__ Cand mine_after(const T* __restrict__ x, int lo, int hv, int hi, Cand prev) {
  Cand a{-INFINITY, kNone};
  for_mine<T>(x, lo, hv, hi, [&](float v, int i) {
    const Cand c{v, i};
    if (before(prev, c)) a = best(a, c);
  });
  return a;
}

// grid (B, P): part blockIdx.y of row blockIdx.x -> pm / ps[row * P + part] and the part's first
// min(want[row], kLpMaxTop) candidates in cv / ci[(row * P + part) * kLpMaxTop ...], sorted; a list
// the part cannot fill ends in {-inf, kNone}.
template <typename T>
__global__ __launch_bounds__(kLT) void logprob_partial_kernel(float* __restrict__ pm, float* __restrict__ ps,
                                                              float* __restrict__ cv, int* __restrict__ ci,
                                                              const T* __restrict__ logits, long stride, int V, int P,
                                                              const int* __restrict__ want) {
  __shared__ float sv[kLT / 64];
  __shared__ int si[kLT / 64];
  const int row = blockIdx.x, part = blockIdx.y;
  const int n = min(want[row], kLpMaxTop);
  if (n < 0) return;  // row-uniform: the row did not ask
  const T* x = logits + (long)row * stride;
  const int chunk = ((V + P - 1) / P + 7) & ~7;
  const int lo = min(V, part * chunk), hi = min(V, lo + chunk);
  const bool vec = std::is_same<T, bf16_t>::value && (stride & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(x + lo) & 15) == 0;
  const int hv = vec ? lo + ((hi - lo) & ~7) : lo;
  const int tid = threadIdx.x;
  const long o = (long)row * P + part;
  cv += o * kLpMaxTop;
  ci += o * kLpMaxTop;

  // round 0 of the selection is the part's maximum
  Cand mine = mine_after<T>(x, lo, hv, hi, Cand{INFINITY, -1});
  Cand win = block_best(mine, sv, si);
  const float m = win.v;
  const float mm = m == -INFINITY ? 0.f : m;  // an all -inf (or empty) part: every term exp(-inf) = 0
  float s = 0.f;
  for_mine<T>(x, lo, hv, hi, [&](float v, int) { s += __expf(v - mm); });
  s = block_sum<kLT>(s, sv);
  if (tid == 0) {
    pm[o] = m;
    ps[o] = s;
  }
  for (int r = 0; r < n; ++r) {
    if (r > 0) {
      if (win.i != kNone) {  // (workgroup-uniform) after "none" comes "none"
        if (mine.i == win.i) mine = mine_after<T>(x, lo, hv, hi, win);
        win = block_best(mine, sv, si);
      }
    }
    if (tid == 0) {
      cv[r] = win.v;
      ci[r] = win.i;
    }
  }
}

// one wave per row: lse from the P (max, sum) pairs in part order, the top n of the P sorted
// lists, x[tok[row]], and the row's record: word 0 = bits of lp(tok), words 1..20 = bits of the
// alternatives' logprobs, words 21..40 = their ids (-1 / -inf past min(n, V)).
// The merge holds one sorted list per lane in registers (every load of it independent of the
// others: one memory latency, not one per round): a round is a wave argmax over the lists' heads,
// and the lane that owned the winner shifts its list down by one.  Lanes 0..62 take a part each;
// with more than 63 parts the merged list so far is lane 63's list of the next pass.
template <typename T>
__global__ __launch_bounds__(64) void logprob_final_kernel(int* __restrict__ out, const float* __restrict__ pm,
                                                           const float* __restrict__ ps, const float* __restrict__ cv,
                                                           const int* __restrict__ ci, const T* __restrict__ logits,
                                                           long stride, int V, int P, const int* __restrict__ tok,
                                                           const int* __restrict__ want) {
  __shared__ float carry_v[kLpMaxTop];
  __shared__ int carry_i[kLpMaxTop];
  const int row = blockIdx.x, lane = threadIdx.x;
  const int n = min(want[row], kLpMaxTop);
  if (n < 0) return;
  const int t = tok[row];
  const bool t_ok = (unsigned)t < (unsigned)V;
  const float xt = t_ok ? ldx<T>(logits + (long)row * stride, t) : 0.f;  // in flight during the merge
  pm += (long)row * P;
  ps += (long)row * P;
  cv += (long)row * P * kLpMaxTop;
  ci += (long)row * P * kLpMaxTop;
  float m = -INFINITY;
  for (int j = 0; j < P; ++j) m = fmaxf(m, pm[j]);
  const float mm = m == -INFINITY ? 0.f : m;
  float s = 0.f;
  for (int j = 0; j < P; ++j) s += ps[j] * __expf(pm[j] - mm);
  const float lse = mm + logf(s);

  Cand res{-INFINITY, kNone};  // lane r: the r-th of the merged list
  for (int base = 0; base < P; base += 63) {
    const int j = base + lane;
    const bool has_part = lane < 63 && j < P, has_carry = lane == 63 && base > 0;
    float lv[kLpMaxTop];
    int li[kLpMaxTop];
#pragma unroll
    for (int r = 0; r < kLpMaxTop; ++r) {
      lv[r] = -INFINITY;
      li[r] = kNone;
      if (r < n) {
        if (has_part) {
          lv[r] = cv[j * kLpMaxTop + r];
          li[r] = ci[j * kLpMaxTop + r];
        } else if (has_carry) {
          lv[r] = carry_v[r];
          li[r] = carry_i[r];
        }
      }
    }
    for (int r = 0; r < n; ++r) {
      const Cand win = wave_best(Cand{lv[0], li[0]});
      if (lane == r) res = win;
      if (li[0] == win.i && win.i != kNone) {
#pragma unroll
        for (int k = 0; k + 1 < kLpMaxTop; ++k) {
          lv[k] = lv[k + 1];
          li[k] = li[k + 1];
        }
        lv[kLpMaxTop - 1] = -INFINITY;
        li[kLpMaxTop - 1] = kNone;
      }
    }
    if (base + 63 < P) {  // wave-uniform: another pass follows
      __syncthreads();
      if (lane < kLpMaxTop) {
        carry_v[lane] = res.v;
        carry_i[lane] = res.i;
      }
      __syncthreads();
    }
  }
  out += (long)row * kLpWidth;
  if (lane < kLpMaxTop) {
    out[1 + lane] = __float_as_int(res.i != kNone ? res.v - lse : -INFINITY);
    out[1 + kLpMaxTop + lane] = res.i != kNone ? res.i : -1;
  }
  if (lane == 0) out[0] = __float_as_int(t_ok ? xt - lse : __int_as_float(0x7fc00000));
}

}  // namespace
}  // namespace k8sllm

using namespace k8sllm;

extern "C" int k8sllm_sample_parts(long B, int V);

// words of workspace k8sllm_token_logprobs needs for B rows of V logits
extern "C" long k8sllm_token_logprobs_ws(long B, int V) {
  return B * k8sllm_sample_parts(B, V) * (2 + 2 * kLpMaxTop);
}

// out int32 [B][41] (rows with want < 0 are not written), tok / want int32 [B], ws: 4-byte words
extern "C" int k8sllm_token_logprobs(int* out, const void* logits, int is_fp32, long B, long stride, int V,
                                     const int* tok, const int* want, void* ws, hipStream_t s) {
  if (want == nullptr || tok == nullptr || out == nullptr || logits == nullptr || ws == nullptr || V <= 0)
    return (int)hipErrorInvalidValue;
  if (B <= 0) return 0;
  const int P = k8sllm_sample_parts(B, V);
  const long np = B * P;
  float* pm = (float*)ws;
  float* ps = pm + np;
  float* cv = ps + np;
  int* ci = (int*)(cv + np * kLpMaxTop);
  dim3 grid((unsigned)B, P);
  if (is_fp32) {
    hipLaunchKernelGGL(logprob_partial_kernel<float>, grid, dim3(kLT), 0, s, pm, ps, cv, ci, (const float*)logits,
                       stride, V, P, want);
    hipLaunchKernelGGL(logprob_final_kernel<float>, dim3((unsigned)B), dim3(64), 0, s, out, pm, ps, cv, ci,
                       (const float*)logits, stride, V, P, tok, want);
  } else {
    hipLaunchKernelGGL(logprob_partial_kernel<bf16_t>, grid, dim3(kLT), 0, s, pm, ps, cv, ci, (const bf16_t*)logits,
                       stride, V, P, want);
    hipLaunchKernelGGL(logprob_final_kernel<bf16_t>, dim3((unsigned)B), dim3(64), 0, s, out, pm, ps, cv, ci,
                       (const bf16_t*)logits, stride, V, P, tok, want);
  }
  return (int)hipGetLastError();
}
