// Last-token pooling for embedding requests on gfx950: the final-normed hidden row of a sequence,
// cut to its first `dim` columns and L2-normalised, as fp32.
//
//   dim[r] <= 0      : not an embedding row, e[r] is left as it is
//   1 <= dim[r] <= d : e[r, :dim] = x[r, :dim] / ||x[r, :dim]||_2, e[r, dim:] = 0 (a zero row gives zeros)
//
// One workgroup per row, as the norms of norm_act.hip.  A step has at most a few dozen embedding
// rows of at most some tens of KB, so the kernel is launch-bound: the row is read twice (the second
// pass hits the cache) instead of being kept in registers, which leaves one form for every width.
// Sums are fp32: per thread in column order, a wave64 butterfly, then the waves' sums through LDS
// in wave order - no atomics, two launches give the same bits.
#include "common.h"

namespace k8sllm {

__device__ __forceinline__ void pool_load8(const bf16_t* p, float* f) {
  unpack8(*reinterpret_cast<const uint4*>(p), f);
}
__device__ __forceinline__ void pool_load8(const float* p, float* f) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
__device__ __forceinline__ float pool_load1(const bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ float pool_load1(const float* p) { return *p; }

// x [R][x_stride] (T = bf16_t or float), out fp32 [R][d] contiguous.  Columns [0, nv) go as groups
// of 8 (16-byte loads, 16-byte stores; nv % 8 == 0 and the launcher has checked the alignment of
// both), columns [nv, d) one by one.
template <typename T>
__global__ __launch_bounds__(256) void pool_l2_kernel(float* __restrict__ out, const T* __restrict__ x,
                                                      const int* __restrict__ dim, int d, int nv, long x_stride) {
  __shared__ float red[4];
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const int n = min(dim[row], d);
  if (n <= 0) return;
  const T* xr = x + (long)row * x_stride;
  float ss = 0.f;
  for (int idx = tid * 8; idx < nv && idx < n; idx += 256 * 8) {
    float v[8];
    pool_load8(xr + idx, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += idx + j < n ? v[j] * v[j] : 0.f;
  }
  for (int idx = nv + tid; idx < n; idx += 256) {
    const float v = pool_load1(xr + idx);
    ss += v * v;
  }
  ss = block_sum<256>(ss, red);
  const float inv = ss > 0.f ? rsqrtf(ss) : 0.f;
  float* orow = out + (long)row * d;
  for (int idx = tid * 8; idx < nv; idx += 256 * 8) {
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (idx < n) {
      pool_load8(xr + idx, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = idx + j < n ? v[j] * inv : 0.f;
    }
    *reinterpret_cast<float4*>(orow + idx) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(orow + idx + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
  for (int idx = nv + tid; idx < d; idx += 256) orow[idx] = idx < n ? pool_load1(xr + idx) * inv : 0.f;
}

}  // namespace k8sllm

using namespace k8sllm;

extern "C" {

// x_stride in elements.  The vector path needs 16-byte aligned rows on both sides; a view that is
// not (an odd stride or offset, d % 4 != 0) takes the scalar path for every column.
int k8sllm_pool_l2(float* out, const void* x, int is_fp32, const int* dim, long rows, int d, long x_stride,
                   hipStream_t s) {
  if (d <= 0 || rows < 0 || x_stride < d) return -1;
  if (rows == 0) return 0;
  const long esz = is_fp32 ? 4 : 2;
  const bool aligned = ((uintptr_t)x % 16 == 0) && ((x_stride * esz) % 16 == 0) && ((uintptr_t)out % 16 == 0) &&
                       (d % 4 == 0);
  const int nv = aligned ? d & ~7 : 0;
  if (is_fp32)
    hipLaunchKernelGGL(pool_l2_kernel<float>, dim3(rows), dim3(256), 0, s, out, (const float*)x, dim, d, nv, x_stride);
  else
    hipLaunchKernelGGL(pool_l2_kernel<bf16_t>, dim3(rows), dim3(256), 0, s, out, (const bf16_t*)x, dim, d, nv,
                       x_stride);
  return (int)hipGetLastError();
}

}  // extern "C"
