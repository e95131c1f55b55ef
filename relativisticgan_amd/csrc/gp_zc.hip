// Zero-centred gradient penalties (R1 on real samples, R2 on generated ones) for gfx950:
// the penalty head ZC(g; gamma) = gamma / 2 * sum_b ||g_b||^2 / n_global on the gradient
// image g of D, and its backward dZC/dg = gamma / n_global * g (not in the reference; the
// one-centred WGAN-GP head of GLI:646-658 is heads_optim.hip's rgan_gp_penalty).
//
// Both kernels stream g once at HBM rate: 16-byte loads when every sample starts on a
// 16-byte boundary (per % 4 == 0 and an aligned base), dword loads otherwise.  The forward
// is a two-stage sum in a fixed order (no atomics, no cross-block counters): stage 1 splits
// every sample over enough 256-thread blocks to fill the chip and leaves one double per
// block in the workspace; stage 2 (one block) adds each sample's partials in split order and
// then the samples in index order, in double.
#include <algorithm>

#include "common.h"

namespace rgan {

constexpr int ZC_THREADS = 256;
constexpr int ZC_BLOCKS = 2048;           // 256 CUs x 8 resident 256-thread blocks
constexpr long long ZC_MIN_CHUNK = 2048;  // floats per block below which a split only adds launches' worth of tail
constexpr int ZC_MAX_BATCH = 65535;       // stage 1 puts the sample index in gridDim.y

// blocks per sample and the floats each one sums (a multiple of 4 * ZC_THREADS, so a
// chunk of a 16-byte aligned sample starts 16-byte aligned); every block gets >= 1 element
static int zc_split(int batch, long long per, long long* chunk) {
  const long long want = std::max<long long>(1, (ZC_BLOCKS + batch - 1) / batch);
  const long long most = std::max<long long>(1, (per + ZC_MIN_CHUNK - 1) / ZC_MIN_CHUNK);
  const long long n = std::min(want, most);
  const long long unit = 4 * ZC_THREADS;
  const long long c = ((per + n - 1) / n + unit - 1) / unit * unit;
  *chunk = c;
  return (int)((per + c - 1) / c);
}

static bool zc_args_ok(int batch, long long per, int n_global) {
  return batch > 0 && batch <= ZC_MAX_BATCH && per > 0 && n_global >= batch;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// part[b * gridDim.x + k] = sum of g_b^2 over chunk k of sample b
__global__ __launch_bounds__(ZC_THREADS) void gp_zc_partial_kernel(const float* __restrict__ g, long long per,
                                                                   long long chunk, int vec,
                                                                   double* __restrict__ part) {
  __shared__ double red[16];
  const float* gb = g + (long long)blockIdx.y * per;
  const long long lo = (long long)blockIdx.x * chunk;
  const long long hi = lo + chunk < per ? lo + chunk : per;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (vec) {  // per % 4 == 0: hi - lo is a multiple of 4 and gb + lo is 16-byte aligned
    const float4* v = reinterpret_cast<const float4*>(gb + lo);
    const long long n4 = (hi - lo) >> 2;
#pragma unroll 4
    for (long long i = threadIdx.x; i < n4; i += ZC_THREADS) {
      const float4 q = v[i];
      a0 = fmaf(q.x, q.x, a0);
      a1 = fmaf(q.y, q.y, a1);
      a2 = fmaf(q.z, q.z, a2);
      a3 = fmaf(q.w, q.w, a3);
    }
  } else {
#pragma unroll 4
    for (long long i = lo + threadIdx.x; i < hi; i += ZC_THREADS) a0 = fmaf(gb[i], gb[i], a0);
  }
  const double s = block_sum_d(((double)a0 + (double)a1) + ((double)a2 + (double)a3), red);
  if (threadIdx.x == 0) part[(long long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// sq[b] = sum_k part[b][k] (k ascending); loss = gamma / 2 * (sum_b sq[b], b ascending) / n_global
__global__ __launch_bounds__(ZC_THREADS) void gp_zc_finish_kernel(const double* __restrict__ part, int batch,
                                                                  int nsplit, float gamma, int n_global,
                                                                  float* __restrict__ sq, float* __restrict__ loss) {
  __shared__ double tile[ZC_THREADS];
  double total = 0.0;  // thread 0's
  for (int b0 = 0; b0 < batch; b0 += ZC_THREADS) {
    const int b = b0 + threadIdx.x;
    double s = 0.0;
    if (b < batch) {
      const double* pb = part + (long long)b * nsplit;
      for (int k = 0; k < nsplit; ++k) s += pb[k];
      sq[b] = (float)s;
    }
    tile[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = batch - b0 < ZC_THREADS ? batch - b0 : ZC_THREADS;
      for (int i = 0; i < n; ++i) total += tile[i];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(0.5 * (double)gamma * total / (double)n_global);
}

// dg may alias g exactly (the GP engine rewrites the gradient image in place): each thread
// reads its elements of g and then writes the same elements of dg, so neither pointer is
// __restrict__
__global__ __launch_bounds__(ZC_THREADS) void gp_zc_bwd_kernel(const float* g, long long total, int vec, float gamma,
                                                               int n_global, const float* __restrict__ gscale,
                                                               float* dg) {
  const float coef = (gscale ? gscale[0] : 1.f) * gamma / (float)n_global;
  const long long start = blockIdx.x * (long long)ZC_THREADS + threadIdx.x;
  const long long step = (long long)gridDim.x * ZC_THREADS;
  if (vec) {  // total % 4 == 0, g and dg 16-byte aligned
    const float4* gv = reinterpret_cast<const float4*>(g);
    float4* dv = reinterpret_cast<float4*>(dg);
    for (long long i = start; i < (total >> 2); i += step) {
      float4 q = gv[i];
      q.x *= coef;
      q.y *= coef;
      q.z *= coef;
      q.w *= coef;
      dv[i] = q;
    }
  } else {
    for (long long i = start; i < total; i += step) dg[i] = coef * g[i];
  }
}

}  // namespace rgan

using namespace rgan;

extern "C" size_t rgan_gp_zc_workspace(int batch, long long per) {
  if (!zc_args_ok(batch, per, batch)) return 0;
  long long chunk;
  return (size_t)batch * (size_t)zc_split(batch, per, &chunk) * sizeof(double);
}

extern "C" int rgan_gp_zc_penalty(const float* g, int batch, long long per, float gamma, int n_global, float* sq,
                                  float* loss, void* ws, void* stream) {
  RGAN_REQUIRE(g && sq && loss && zc_args_ok(batch, per, n_global));
  RGAN_REQUIRE(ws);  // rgan_gp_zc_workspace is nonzero for every accepted (batch, per)
  hipStream_t s = (hipStream_t)stream;
  long long chunk;
  const int nsplit = zc_split(batch, per, &chunk);
  const int vec = per % 4 == 0 && aligned16(g);
  gp_zc_partial_kernel<<<dim3(nsplit, batch), ZC_THREADS, 0, s>>>(g, per, chunk, vec, (double*)ws);
  RGAN_CHECK_LAUNCH();
  gp_zc_finish_kernel<<<1, ZC_THREADS, 0, s>>>((const double*)ws, batch, nsplit, gamma, n_global, sq, loss);
  RGAN_CHECK_LAUNCH();
  return 0;
}

extern "C" int rgan_gp_zc_penalty_backward(const float* g, int batch, long long per, float gamma, int n_global,
                                           const float* gscale, float* dg, void* stream) {
  RGAN_REQUIRE(g && dg && zc_args_ok(batch, per, n_global));
  const long long total = (long long)batch * per;
  const int vec = per % 4 == 0 && aligned16(g) && aligned16(dg);
  const long long items = vec ? total >> 2 : total;
  const int grid = (int)std::min<long long>((items + ZC_THREADS - 1) / ZC_THREADS, 2 * ZC_BLOCKS);
  gp_zc_bwd_kernel<<<grid, ZC_THREADS, 0, (hipStream_t)stream>>>(g, total, vec, gamma, n_global, gscale, dg);
  RGAN_CHECK_LAUNCH();
  return 0;
}
