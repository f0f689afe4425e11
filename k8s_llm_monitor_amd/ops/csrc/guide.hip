// Constrained decoding: the per-state token masks of a guide (ops.GuideState, engine/guide.py).
//
// A guide is a DFA over bytes whose n states live in rows of a device arena: trans [rows][256]
// holds absolute row numbers (-1 = dead), accept [rows] one byte per row.  The vocabulary is CSR
// (tok_off [V + 1], a byte blob).  mask [rows][W] (W words of 32 bits, a multiple of 4 so every row
// is 16-byte aligned) gets bit t & 31 of word t >> 5 set iff a row in that state may draw token t
// (ops/reference.py guide_mask):
//   - t has at least one byte and walking its bytes from the state never hits -1;
//   - t is an eos id: iff the state accepts;
//   - bits at and past V (the padding of the last words) are 0.
//
// guide_mask_build_kernel, decomposition: token-major.  A thread owns one token and walks it from
// kGS states in turn; a workgroup is 4 waves x 64 consecutive tokens, grid (ceil(32 W / 256),
// ceil(n / kGS)).  The token's first kGReg bytes are loaded once into four registers and reused
// for every state (a longer token reads its tail from the blob, an L2 hit, per state); the walk's
// dependent loads go to trans, which is 1 KB per state - 512 KB for a full 512-state guide, L2
// resident.  A wave ballot packs its 64 verdicts into two words that lane 0 writes with one
// 8-byte vector store: every word of the mask is written exactly once, no atomics, the same
// bits on every launch.  guide_row_popc_kernel then counts each row (one workgroup per row), so
// the host can refuse a guide with a non-accepting state nobody can leave.
//
// Measured on an MI355X (profiles/r22/README.md): a 512-state guide over the 128256-token
// vocabulary of the built-in tokenizer (496 KB of token bytes, the longest token 336 bytes), both
// kernels together 0.205 .. 0.215 ms - 65.7 M walks and 8.2 MB of mask; GuideState.load as a whole
// (two uploads, two scatters, the two kernels) 0.9 .. 1.0 ms on the stream.  This is the only
// decomposition that was built and measured; a state-major one (a workgroup per state with its
// trans row in LDS) would save nothing on the first lookup and has every later lookup leave the
// row anyway.  44 VGPRs, no scratch (guide_row_popc_kernel: 6).
#include "common.h"

namespace k8sllm {

constexpr int kGT = 256;   // threads per workgroup
constexpr int kGS = 16;    // states a thread walks its token from
constexpr int kGReg = 16;  // token bytes held in registers

__global__ __launch_bounds__(kGT) void guide_mask_build_kernel(uint32_t* __restrict__ mask, int W,
                                                               const int* __restrict__ trans,
                                                               const uint8_t* __restrict__ accept,
                                                               const int* __restrict__ rows, int n, int nrows,
                                                               const int* __restrict__ tok_off,
                                                               const uint8_t* __restrict__ blob, int V,
                                                               const int* __restrict__ eos_ids, int n_eos) {
  const int t = blockIdx.x * kGT + threadIdx.x;
  const int word = (t >> 6) * 2;  // wave-uniform: the wave's two words
  if (word >= W) return;          // W is even: both words or none
  int len = 0;
  long off = 0;
  bool eos = false;
  uint32_t r[kGReg / 4] = {0u, 0u, 0u, 0u};
  if (t < V) {
    off = tok_off[t];
    len = tok_off[t + 1] - (int)off;
#pragma unroll
    for (int j = 0; j < kGReg; ++j)
      if (j < len) r[j >> 2] |= (uint32_t)blob[off + j] << (8 * (j & 3));
    for (int e = 0; e < n_eos; ++e) eos |= eos_ids[e] == t;
  }
  const int s0 = blockIdx.y * kGS, s1 = min(n, s0 + kGS);
  for (int si = s0; si < s1; ++si) {
    const int row = rows[si];
    if ((unsigned)row >= (unsigned)nrows) continue;  // uniform; the host never passes one
    bool ok;
    if (eos) {
      ok = accept[row] != 0;
    } else {
      int s = row;
#pragma unroll
      for (int j = 0; j < kGReg; ++j)
        if (j < len && (unsigned)s < (unsigned)nrows) s = trans[(long)s * 256 + ((r[j >> 2] >> (8 * (j & 3))) & 0xffu)];
      for (int j = kGReg; j < len && (unsigned)s < (unsigned)nrows; ++j) s = trans[(long)s * 256 + blob[off + j]];
      ok = len > 0 && (unsigned)s < (unsigned)nrows;
    }
    const unsigned long long b = __ballot(ok);
    if ((threadIdx.x & 63) == 0)
      *reinterpret_cast<uint2*>(mask + (long)row * W + word) = make_uint2((uint32_t)b, (uint32_t)(b >> 32));
  }
}

// popc[rows[i]] = the number of allowed tokens of that row; one workgroup per row
__global__ __launch_bounds__(kGT) void guide_row_popc_kernel(int* __restrict__ popc, const uint32_t* __restrict__ mask,
                                                             int W, const int* __restrict__ rows, int nrows) {
  __shared__ float red[kGT / 64];
  const int row = rows[blockIdx.x];
  if ((unsigned)row >= (unsigned)nrows) return;
  float c = 0.f;  // 32 W < 2^24: an exact count
  for (int i = threadIdx.x; i < W; i += kGT) c += (float)__popc(mask[(long)row * W + i]);
  c = block_sum<kGT>(c, red);
  if (threadIdx.x == 0) popc[row] = (int)c;
}

}  // namespace k8sllm

using namespace k8sllm;

// rows [n]: the guide's absolute rows (device memory), state i of the guide in rows[i]
extern "C" int k8sllm_guide_mask_build(void* mask, int W, const int* trans, const void* accept, int* popc,
                                       const int* rows, int n, int nrows, const int* tok_off, const void* blob, int V,
                                       const int* eos_ids, int n_eos, hipStream_t s) {
  if (n <= 0) return 0;
  if (W <= 0 || (W & 3) != 0 || (long)W * 32 < V || nrows <= 0 || n_eos < 0 ||
      (reinterpret_cast<uintptr_t>(mask) & 15) != 0)
    return (int)hipErrorInvalidValue;
  dim3 grid((unsigned)((W * 32 + kGT - 1) / kGT), (unsigned)((n + kGS - 1) / kGS));
  hipLaunchKernelGGL(guide_mask_build_kernel, grid, dim3(kGT), 0, s, (uint32_t*)mask, W, trans, (const uint8_t*)accept,
                     rows, n, nrows, tok_off, (const uint8_t*)blob, V, eos_ids, n_eos);
  hipLaunchKernelGGL(guide_row_popc_kernel, dim3((unsigned)n), dim3(kGT), 0, s, popc, (const uint32_t*)mask, W, rows,
                     nrows);
  return (int)hipGetLastError();
}
