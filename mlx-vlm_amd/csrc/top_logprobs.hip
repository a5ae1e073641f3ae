// top_logprobs: the K best log-probs of a vocabulary row, as the reference's batch generator reports them
// (mlx_vlm/generate/ar.py:1092-1122):
//   sort_idx = argsort(logprobs)            ascending
//   top_idx  = sort_idx[..., -k:][..., ::-1]
//   top_lp   = take_along_axis(logprobs, top_idx)
// i.e. value descending and, among EQUAL values, the HIGHER index first (a stable ascending sort puts the lower index first
// among equals and the slice is reversed; oracle/mlx_shim states argsort as torch.argsort(stable=True) - whether MLX's own
// argsort is stable could not be checked against MLX itself: parity unpinned).  The comparison is on values: +0.0 and -0.0
// tie and the index decides; -inf entries are ordinary values that tie with each other; NaN is outside the contract.
//
// That order is a TOTAL order on (value key, index): every element gets the 48-bit composite (key << 32) | index with key
// the order-preserving 16-bit image of the bf16 value (-0 folded onto +0), all composites of a row are distinct, and the
// answer is the K largest composites in descending order.  Ties - a bf16 row of 151,936 log-probs holds ~235 distinct
// values - need no separate rule.
//
// One 1024-thread workgroup per row, no workspace, the input row is only read:
//   1  every thread takes the maximum composite of its elements; lane group g (the threads with tid % 64 == g) holds one
//      distinct element >= the smallest of the 64 group maxima L, so the K <= 64 best are all >= L;
//   2  the elements >= L (about 64 H_64 ~ 300 of a row in random order; ~600 of an all-equal row, where the order is the
//      index order and consecutive 16-byte chunks go to consecutive groups) are appended to a list in LDS;
//   3  radix select of the K-th largest composite T over the list: six 8-bit digits from the top, a 256-bin LDS histogram
//      per digit (lanes of a wave that hold the same digit add once);
//   4  the K elements >= T are ranked by one wavefront (rank = composites above mine) and written with the row's own bits
//      at their index (-0.0 stays -0.0).
// A row laid out against the thread assignment (all large values in a few lane groups) can put more than TLP_CAP elements
// above L: steps 3 and 4 then run over the row itself (seven more passes) instead of the list - same result, only slower.
#include "common.hpp"
#include "internal.h"

namespace {

constexpr int TLP_MAX_K = 64;
constexpr int TLP_CAP = 2048;       // list entries in LDS (16 KB)

// the value order of bf16 bits as an ascending 16-bit key; +0.0 and -0.0 share a key
__device__ __forceinline__ uint32_t value_key(uint32_t b) {
  if ((b & 0x7fffu) == 0u) b = 0u;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
__device__ __forceinline__ unsigned long long composite(uint32_t bits, int i) {
  return ((unsigned long long)value_key(bits) << 32) | (unsigned long long)(uint32_t)i;
}

// f(in, index, bits) for every element of the row; every lane of the workgroup makes the same number of calls (`in` false
// past the end), so f may use wavefront ballots.  16-byte loads when the row is aligned, one element per lane otherwise.
template <typename F>
__device__ __forceinline__ void row_each(const bf16_t* __restrict__ row, int V, bool vec, F f) {
  const int tid = threadIdx.x;
  if (vec) {
    const int V8 = V >> 3;
    for (int c0 = 0; c0 < V8; c0 += 1024) {
      const int c = c0 + tid;
      const bool in = c < V8;
      u32x4_t w = {0u, 0u, 0u, 0u};
      if (in) w = *reinterpret_cast<const u32x4_t*>(row + (size_t)c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) f(in, c * 8 + e, (e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu));
    }
    if (V & 7) {
      const int i = (V8 << 3) + tid;
      const bool in = i < V;
      f(in, i, in ? (uint32_t)row[i] : 0u);
    }
  } else {
    for (int i0 = 0; i0 < V; i0 += 1024) {
      const int i = i0 + tid;
      const bool in = i < V;
      f(in, i, in ? (uint32_t)row[i] : 0u);
    }
  }
}

// hist[bin] += 1 for the lanes with `hit`; called by every lane of the wavefront.  Lanes that all hold the same bin (an
// all-equal row: 150,000 additions to one word would serialise) add once.
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t bin, bool hit) {
  const unsigned long long active = __ballot(hit);
  if (!active) return;
  const int leader = __ffsll((long long)active) - 1;
  const uint32_t first = (uint32_t)__shfl((int)bin, leader, 64);
  const unsigned long long same = __ballot(hit && bin == first);
  if (same == active) {
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[first], (uint32_t)__popcll(active));
  } else if (hit) {
    atomicAdd(&hist[bin], 1u);
  }
}

__global__ __launch_bounds__(1024) void top_logprobs_kernel(const bf16_t* __restrict__ lp, int ld, int V, int K,
                                                            int* __restrict__ out_idx, bf16_t* __restrict__ out_val) {
  __shared__ unsigned long long s_cand[TLP_CAP];      // first the threads' maxima [1024], then the list
  __shared__ unsigned long long s_top[TLP_MAX_K];
  __shared__ unsigned long long s_bound;
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_n, s_m, s_digit, s_rem;
  const int b = blockIdx.x, tid = threadIdx.x;
  const bf16_t* row = lp + (size_t)b * ld;
  const bool vec = ((uintptr_t)row & 15) == 0;

  // ---- 1: L = the smallest of the 64 lane groups' maxima
  unsigned long long mx = 0ull;
  row_each(row, V, vec, [&](bool in, int i, uint32_t bits) {
    const unsigned long long c = composite(bits, i);
    if (in && c > mx) mx = c;
  });
  s_cand[tid] = mx;
  if (tid == 0) { s_n = 0u; s_m = 0u; s_digit = 0u; s_rem = 1u; }
  if (tid < TLP_MAX_K) s_top[tid] = 0ull;
  __syncthreads();
  if (tid < 64) {
    unsigned long long g = 0ull;
    for (int w = 0; w < 16; ++w) { const unsigned long long t = s_cand[tid + 64 * w]; g = t > g ? t : g; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(g >> 32), o, 64), lo = (uint32_t)__shfl_xor((int)(uint32_t)g, o, 64);
      const unsigned long long t = ((unsigned long long)hi << 32) | lo;
      g = t < g ? t : g;
    }
    if (tid == 0) s_bound = g;      // (a group without an element - V < 64 - has maximum 0: every element is kept)
  }
  __syncthreads();
  const unsigned long long L = s_bound;

  // ---- 2: the elements >= L, in any order
  row_each(row, V, vec, [&](bool in, int i, uint32_t bits) {
    const unsigned long long c = composite(bits, i);
    if (in && c >= L) {
      const uint32_t at = atomicAdd(&s_n, 1u);
      if (at < (uint32_t)TLP_CAP) s_cand[at] = c;
    }
  });
  __syncthreads();
  const uint32_t n = s_n;
  const bool listed = n <= (uint32_t)TLP_CAP;       // (uniform)
  // f(in, composite) over the elements >= L: the list, or the row when the list overflowed
  auto each = [&](auto f) {
    if (listed) {
      for (uint32_t j0 = 0; j0 < n; j0 += 1024) {
        const uint32_t j = j0 + (uint32_t)tid;
        const bool in = j < n;
        f(in, in ? s_cand[j] : 0ull);
      }
    } else {
      row_each(row, V, vec, [&](bool in, int i, uint32_t bits) {
        const unsigned long long c = composite(bits, i);
        f(in && c >= L, c);
      });
    }
  };

  // ---- 3: T = the K-th largest composite, digit by digit: among the elements that share the digits found so far, the
  // digit d with (elements of a larger digit) < rem <= (elements of digit >= d)
  unsigned long long prefix = 0ull;
  uint32_t rem = (uint32_t)K;
  for (int shift = 40; shift >= 0; shift -= 8) {
    if (tid < 256) s_hist[tid] = 0u;
    __syncthreads();
    each([&](bool in, unsigned long long c) { hist_add(s_hist, (uint32_t)(c >> shift) & 255u, in && (c >> (shift + 8)) == prefix); });
    __syncthreads();
    if (tid < 64) {
      uint32_t bins[4], s = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) { bins[j] = s_hist[4 * tid + j]; s += bins[j]; }
      uint32_t suf = s;                                   // elements in this lane's bins and the higher lanes'
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_down((int)suf, o, 64);
        if (tid + o < 64) suf += t;
      }
      uint32_t above = suf - s;
      if (above < rem && rem <= suf) {
        for (int j = 3; j >= 0; --j) {
          if (above + bins[j] >= rem) { s_digit = 4u * (uint32_t)tid + (uint32_t)j; s_rem = rem - above; break; }
          above += bins[j];
        }
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | (unsigned long long)s_digit;
    rem = s_rem;
  }
  const unsigned long long T = prefix;

  // ---- 4: the K elements >= T, ranked by one wavefront
  each([&](bool in, unsigned long long c) {
    if (in && c >= T) {
      const uint32_t at = atomicAdd(&s_m, 1u);
      if (at < (uint32_t)TLP_MAX_K) s_top[at] = c;
    }
  });
  __syncthreads();
  if (tid < K) {
    const unsigned long long mine = s_top[tid];
    int rank = 0;
    for (int j = 0; j < K; ++j) rank += s_top[j] > mine;
    const int i = min((int)(uint32_t)mine, V - 1);
    out_idx[(size_t)b * K + rank] = i;
    out_val[(size_t)b * K + rank] = row[i];
  }
}

}  // namespace

// lp bf16 [B][ld] (ld >= V; what lies past V is never read) -> idx int32 [B][K], val bf16 [B][K] (the row's own bits at
// idx), 1 <= K <= min(64, V).  Reached through vlm_sample_ex(input_is_logprobs == 2), include/vlm_hip.h.
VLM_INTERNAL int vlm_top_logprobs(const void* lp, int ld, int B, int V, int K, void* idx, void* val, void* stream) {
  if (!lp || !idx || !val || B <= 0 || V <= 0) return VLM_ERR_ARG;
  if (K < 1 || K > TLP_MAX_K || K > V || ld < V) return VLM_ERR_SHAPE;
  hipLaunchKernelGGL(top_logprobs_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, (const bf16_t*)lp, ld, V, K, (int*)idx,
                     (bf16_t*)val);
  VLM_CHECK_LAUNCH();
  return VLM_OK;
}
