// Adaptive augmentation probability for gfx950 (--rgan_ada_target; the reference has no
// counterpart): the overfitting statistic of a D step and the controller that moves the
// probability p that rgan_diffaug_p gates its transforms with.
//
// Statistic: the (real, fake) pairs of a D step that D ranks correctly minus those it ranks
// wrongly, S += #(y_real > y_fake) - #(y_real < y_fake), N += n.  Ties and comparisons with a
// NaN count 0 (both tests are false).  The counts are integers: one block adds its threads'
// counts in a fixed order (no atomics), and S, N stay exact in double up to 2^53, so shards
// of a batch add exactly in any order.
//
// Controller (every interval-th call): r = S / N; p moves by N / images_per_unit_p towards 1
// when r > target, towards 0 when r < target, clamped to [0, 1]; S = N = 0.  All in double.
//
// state = {p, S, N, calls} and hyper = {target, interval, images_per_unit_p, reserved} live in
// device memory (as the moving average's count and beta do, ema.hip): a call captured in a HIP
// graph keeps counting across replays and follows a hyper-parameter written between them.
#include "common.h"

namespace rgan {

__device__ __forceinline__ void ada_adjust(const double* __restrict__ hyper, double* __restrict__ state) {
  const double calls = state[3] + 1.0;
  state[3] = calls;
  const double N = state[2];
  if (!(fmod(calls, hyper[1]) == 0.0) || !(N > 0.0)) return;  // (an interval of 0 or NaN never adjusts)
  const double d = state[1] / N - hyper[0];
  const double step = N / hyper[2];
  double p = state[0];
  if (d > 0.0) p += step;
  else if (d < 0.0) p -= step;
  state[0] = p < 0.0 ? 0.0 : (p > 1.0 ? 1.0 : p);
  state[1] = 0.0;
  state[2] = 0.0;
}

__global__ __launch_bounds__(256) void ada_update_kernel(const float* __restrict__ y_real,
                                                         const float* __restrict__ y_fake, int n,
                                                         const double* __restrict__ hyper,
                                                         double* __restrict__ state, int adjust) {
  __shared__ int red[4];
  int acc = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float a = y_real[i], b = y_fake[i];
    acc += (a > b ? 1 : 0) - (a < b ? 1 : 0);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    state[1] += (double)(red[0] + red[1] + red[2] + red[3]);
    state[2] += (double)n;
    if (adjust) ada_adjust(hyper, state);
  }
}

__global__ void ada_adjust_kernel(const double* __restrict__ hyper, double* __restrict__ state) {
  if (threadIdx.x == 0 && blockIdx.x == 0) ada_adjust(hyper, state);
}

}  // namespace rgan

using namespace rgan;

extern "C" int rgan_ada_update(const float* y_real, const float* y_fake, int n, const double* hyper, double* state,
                               int adjust, void* stream) {
  RGAN_REQUIRE(y_real && y_fake && hyper && state && n > 0);
  ada_update_kernel<<<1, 256, 0, (hipStream_t)stream>>>(y_real, y_fake, n, hyper, state, adjust != 0);
  RGAN_CHECK_LAUNCH();
  return 0;
}

extern "C" int rgan_ada_adjust(const double* hyper, double* state, void* stream) {
  RGAN_REQUIRE(hyper && state);
  ada_adjust_kernel<<<1, 64, 0, (hipStream_t)stream>>>(hyper, state);
  RGAN_CHECK_LAUNCH();
  return 0;
}
