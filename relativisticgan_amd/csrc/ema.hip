// Exponential moving average of the generator's weights for gfx950 (--rgan_ema_G; the reference
// has no counterpart).  One multi-tensor streaming update per G step:
//   count += 1;  t = count;  beta_t = warmup ? min(beta, (1 + t) / (10 + t)) : beta   (double)
//   w = (float)(1 - beta_t);  avg = lerp(avg, p, w)                                    (fp32)
// with torch.lerp's two forms (ATen lerp_vec, as adam_elem takes exp_avg): fma(w, p - avg, avg)
// for w < 1/2, fma(w - 1, p - avg, p) otherwise, so w = 1 (beta = 0, or the warm-up's first
// steps with a small beta) returns p itself.  beta, the warm-up switch and the count are read
// from device memory: a captured call follows the counter across replays and a changed beta.
//
// Structure as adam_kernel (heads_optim.hip): tensors chunked into a by-value batch struct, a
// 1-D grid in proportion to size, EMA_BLOCK_ELEMS elements per block, 4 float4 of p and of avg
// in flight per thread.  12 B/element of HBM traffic (read p, read avg, write avg).  A tensor
// whose avg or p is only 4-byte aligned runs the block's elements one float per lane, and so
// does the tail (numel % 4) of an aligned one.
#include "common.h"

#include <algorithm>

namespace rgan {

struct EmaTensor {
  float* avg;
  const float* p;
  long long n;
};
constexpr int EMA_CHUNK = 48;
constexpr int EMA_BLOCK_ELEMS = 4096;
struct EmaBatch {
  EmaTensor t[EMA_CHUNK];
  int first[EMA_CHUNK + 1];  // tensor j owns blocks [first[j], first[j+1])
  int cnt;
};

// hyper = {beta, warmup (0 | 1)}; count = the update being taken (>= 1)
__device__ __forceinline__ float ema_weight(const double* hyper, const float* count) {
  const double beta = hyper[0], t = (double)count[0];
  const double ramp = (1.0 + t) / (10.0 + t);
  const double beta_t = hyper[1] != 0.0 && ramp < beta ? ramp : beta;
  return (float)(1.0 - beta_t);
}

__device__ __forceinline__ float ema_elem(float w, float avg, float p) {
  const float diff = __fsub_rn(p, avg);
  return w < 0.5f ? fmaf(w, diff, avg) : fmaf(w - 1.f, diff, p);
}

__global__ __launch_bounds__(256) void ema_kernel(EmaBatch b, const double* __restrict__ hyper,
                                                  const float* __restrict__ count) {
  int j = 0;
  while (j + 1 < b.cnt && (int)blockIdx.x >= b.first[j + 1]) ++j;
  const EmaTensor T = b.t[j];
  const float w = ema_weight(hyper, count);
  const long long e0 = (long long)((int)blockIdx.x - b.first[j]) * EMA_BLOCK_ELEMS;
  const long long e1 = min(T.n, e0 + EMA_BLOCK_ELEMS);
  const bool vec = (((uintptr_t)T.avg | (uintptr_t)T.p) & 15) == 0;
  // e0 is a multiple of 4, so the float4 body of this block ends at the tensor's last whole float4
  const long long v1 = vec ? (e1 & ~3LL) : e0;
  constexpr int U = EMA_BLOCK_ELEMS / 1024;  // float4 per thread
  float4 P[U], A[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long long i = e0 + 4 * (threadIdx.x + 256 * u);
    if (i < v1) {
      P[u] = *reinterpret_cast<const float4*>(T.p + i);
      A[u] = *reinterpret_cast<const float4*>(T.avg + i);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long long i = e0 + 4 * (threadIdx.x + 256 * u);
    if (i < v1) {
      A[u].x = ema_elem(w, A[u].x, P[u].x);
      A[u].y = ema_elem(w, A[u].y, P[u].y);
      A[u].z = ema_elem(w, A[u].z, P[u].z);
      A[u].w = ema_elem(w, A[u].w, P[u].w);
      *reinterpret_cast<float4*>(T.avg + i) = A[u];
    }
  }
  for (long long i = v1 + threadIdx.x; i < e1; i += 256) T.avg[i] = ema_elem(w, T.avg[i], T.p[i]);
}

}  // namespace rgan

using namespace rgan;

extern "C" int rgan_ema_update(int ntensors, float* const* avg, const float* const* params, const long long* numel,
                               const double* hyper, float* count, void* stream) {
  RGAN_REQUIRE(ntensors >= 0 && hyper && count);
  RGAN_REQUIRE(ntensors == 0 || (avg && params && numel));
  // every tensor checked before the first launch: a refused call changes nothing
  for (int j = 0; j < ntensors; ++j) RGAN_REQUIRE(avg[j] && params[j] && numel[j] >= 0);
  for (int base = 0; base < ntensors; base += EMA_CHUNK) {
    long long blocks = 0;
    for (int j = base; j < std::min(ntensors, base + EMA_CHUNK); ++j) {
      RGAN_REQUIRE(numel[j] <= (1LL << 42));
      blocks += (numel[j] + EMA_BLOCK_ELEMS - 1) / EMA_BLOCK_ELEMS;
    }
    RGAN_REQUIRE(blocks < (1LL << 30));
  }
  if (ntensors == 0) return 0;  // nothing averaged: the count stays
  hipStream_t s = (hipStream_t)stream;
  const int rc = rgan_adam_step_inc(count, stream);  // count[0] += 1, one thread, ahead of the first chunk
  if (rc) return rc;
  for (int base = 0; base < ntensors; base += EMA_CHUNK) {
    const int cnt = std::min(EMA_CHUNK, ntensors - base);
    EmaBatch b{};
    b.cnt = cnt;
    long long blocks = 0;
    for (int i = 0; i < cnt; ++i) {
      const int j = base + i;
      b.t[i] = EmaTensor{avg[j], params[j], numel[j]};
      b.first[i] = (int)blocks;
      blocks += (numel[j] + EMA_BLOCK_ELEMS - 1) / EMA_BLOCK_ELEMS;
    }
    b.first[cnt] = (int)blocks;
    if (blocks == 0) continue;
    ema_kernel<<<(unsigned)blocks, 256, 0, s>>>(b, hyper, count);
    RGAN_CHECK_LAUNCH();
  }
  return 0;
}
