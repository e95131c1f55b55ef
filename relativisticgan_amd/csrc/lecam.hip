// LeCam regularisation of D for gfx950 (--rgan_lecam; Tseng et al., "Regularizing GANs under
// limited data", CVPR 2021; the reference has no counterpart): the distance between D's outputs
// and moving averages ("anchors") of D's outputs on the other kind of batch, its gradients, and
// the move of the anchors, from the two output vectors a D step already holds.
//
// Term (rows i < n of this rank, N = n_global rows over all ranks):
//   w = calls >= start ? lambda : 0                      (calls as it stands before the call)
//   L = w [ (1/N) sum (y_real - a_fake)^2 + (1/N) sum (y_fake - a_real)^2 ]
//   dy_real[i] = (float)(2 w / N (y_real[i] - a_fake));  dy_fake[i] likewise with a_real
// (w == 0: L and the gradients are exact zeros).  Then the anchors move on the batch means
// m = sum y / N: a = m when calls == 0, else beta a + (1 - beta) m; a side that is absent leaves
// its anchor alone, and calls += 1 goes with the fake side.  Everything is double: one block
// adds its threads' sums in a fixed order (no atomics), so two calls on the same inputs give the
// same bits, and each gradient element is rounded once, from double to fp32.
//
// state = {a_real, a_fake, calls, 0} and hyper = {lambda, beta, start, 0} live in device memory
// (as the adaptive probability's do, ada.hip): a call captured in a HIP graph keeps moving the
// anchors across replays and follows a hyper-parameter written between them.
//
// Data parallel: every rank holds the same anchors, so mode 1 writes the gradients (scaled by
// the global N) and the four partial sums {sum y_real, sum y_fake, sum (y_real - a_fake)^2,
// sum (y_fake - a_real)^2} without touching the state; the finish kernel turns the all-reduced
// sums into L and the new anchors.  Mode 0 is both in one launch.
#include "common.h"

namespace rgan {

// sums = {sum y_real, sum y_fake, sum (y_real - a_fake)^2, sum (y_fake - a_real)^2} over the
// global batch; sides: bit 0 the real side is present, bit 1 the fake side
__device__ __forceinline__ void lecam_finish(const double* sums, double N, int sides,
                                             const double* __restrict__ hyper, double* __restrict__ state,
                                             double* loss) {
  const double calls = state[2];
  const double w = calls >= hyper[2] ? hyper[0] : 0.0;
  double L = 0.0;
  if (w != 0.0) {
    if (sides & 1) L += sums[2] / N;
    if (sides & 2) L += sums[3] / N;
    L *= w;
  }
  loss[0] = L;
  const double beta = hyper[1];
  if (sides & 1) {
    const double m = sums[0] / N;
    state[0] = calls == 0.0 ? m : beta * state[0] + (1.0 - beta) * m;
  }
  if (sides & 2) {
    const double m = sums[1] / N;
    state[1] = calls == 0.0 ? m : beta * state[1] + (1.0 - beta) * m;
    state[2] = calls + 1.0;
  }
}

// One side's rows: the gradient of each and this thread's share of the two sums.
__device__ __forceinline__ void lecam_side(const float* __restrict__ y, float* __restrict__ dy, int n, double anchor,
                                           double scale, double& sum, double& sq) {
  for (int i = threadIdx.x; i < n; i += 256) {
    const double v = (double)y[i];
    const double d = v - anchor;
    sum += v;
    sq += d * d;
    if (dy) dy[i] = scale != 0.0 ? (float)(scale * d) : 0.f;
  }
}

__global__ __launch_bounds__(256) void lecam_kernel(const float* __restrict__ y_real,
                                                    const float* __restrict__ y_fake, int n, int n_global,
                                                    const double* __restrict__ hyper, double* __restrict__ state,
                                                    float* __restrict__ dy_real, float* __restrict__ dy_fake,
                                                    double* __restrict__ out, int partial) {
  __shared__ double red[4][4];
  const double a_real = state[0], a_fake = state[1];
  const double w = state[2] >= hyper[2] ? hyper[0] : 0.0;
  const double N = (double)n_global;
  const double scale = w != 0.0 ? 2.0 * w / N : 0.0;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (y_real) lecam_side(y_real, dy_real, n, a_fake, scale, acc[0], acc[2]);
  if (y_fake) lecam_side(y_fake, dy_fake, n, a_real, scale, acc[1], acc[3]);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = wave_sum_d(acc[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();  // (also: every thread has read the anchors before thread 0 moves them)
  if (threadIdx.x == 0) {
    double sums[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) sums[k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
    if (partial) {
#pragma unroll
      for (int k = 0; k < 4; ++k) out[k] = sums[k];
    } else {
      lecam_finish(sums, N, (y_real ? 1 : 0) | (y_fake ? 2 : 0), hyper, state, out);
      out[1] = out[2] = out[3] = 0.0;
    }
  }
}

__global__ void lecam_finish_kernel(const double* sums, int n_global, int sides, const double* __restrict__ hyper,
                                    double* __restrict__ state, double* loss) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const double s[4] = {sums[0], sums[1], sums[2], sums[3]};  // (loss may be sums itself)
    lecam_finish(s, (double)n_global, sides, hyper, state, loss);
  }
}

}  // namespace rgan

using namespace rgan;

extern "C" int rgan_lecam(const float* y_real, const float* y_fake, int n, int n_global, const double* hyper,
                          double* state, float* dy_real, float* dy_fake, double* out, int mode, void* stream) {
  RGAN_REQUIRE(n > 0 && n_global >= n);
  RGAN_REQUIRE(y_real || y_fake);
  RGAN_REQUIRE((y_real || !dy_real) && (y_fake || !dy_fake));
  RGAN_REQUIRE(hyper && state && out);
  RGAN_REQUIRE(mode == 0 || mode == 1);
  lecam_kernel<<<1, 256, 0, (hipStream_t)stream>>>(y_real, y_fake, n, n_global, hyper, state, dy_real, dy_fake, out,
                                                   mode);
  RGAN_CHECK_LAUNCH();
  return 0;
}

extern "C" int rgan_lecam_finish(const double* sums, int n_global, int sides, const double* hyper, double* state,
                                 double* loss, void* stream) {
  RGAN_REQUIRE(sums && hyper && state && loss);
  RGAN_REQUIRE(n_global > 0 && sides >= 1 && sides <= 3);
  lecam_finish_kernel<<<1, 64, 0, (hipStream_t)stream>>>(sums, n_global, sides, hyper, state, loss);
  RGAN_CHECK_LAUNCH();
  return 0;
}
