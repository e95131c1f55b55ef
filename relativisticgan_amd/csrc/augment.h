// Per-sample parameters of --rgan_diffaug shared by csrc/augment.hip (colour, translation,
// cutout) and csrc/augment_geo.hip (x-flip, quarter turns, warp): both derive them from the
// same rows of uniforms by the same rules, so a group that is closed or cleared means the same
// thing in either file.
#pragma once
#include "common.h"

#include <algorithm>

namespace rgan {

struct AugParam {
  float beta, sat, con;
  int tx, ty;          // source of output (i, j) is (i + tx, j + ty)
  int r0, r1, c0, c1;  // cutout box, inclusive (empty: r1 < r0)
};

// min(floor(u n), n - 1), clamped below too (u is caller data: every index derived from it
// stays in range whatever it holds).  The product is exact in double.
__device__ __forceinline__ int aug_pick(float u, int n) {
  const int v = (int)floor((double)u * (double)n);
  return v < 0 ? 0 : (v > n - 1 ? n - 1 : v);
}

__device__ __forceinline__ AugParam aug_param(const float* __restrict__ u, int b, int H, int W, int policy) {
  const float* r = u + 8LL * b;
  AugParam p;
  const bool colour = policy & 1;
  p.beta = colour ? r[0] - 0.5f : 0.f;
  p.sat = colour ? 2.f * r[1] : 1.f;
  p.con = colour ? r[2] + 0.5f : 1.f;
  p.tx = p.ty = 0;
  if (policy & 2) {
    const int Rh = (H + 4) / 8, Rw = (W + 4) / 8;  // floor(H / 8 + 1/2)
    p.tx = aug_pick(r[3], 2 * Rh + 1) - Rh;
    p.ty = aug_pick(r[4], 2 * Rw + 1) - Rw;
  }
  p.r0 = p.c0 = 0;
  p.r1 = p.c1 = -1;
  if (policy & 4) {
    const int Kh = (H + 1) / 2, Kw = (W + 1) / 2;  // floor(H / 2 + 1/2)
    p.r0 = aug_pick(r[5], H + 1 - (Kh & 1)) - Kh / 2;
    p.r1 = p.r0 + Kh - 1;
    p.c0 = aug_pick(r[6], W + 1 - (Kw & 1)) - Kw / 2;
    p.c1 = p.c0 + Kw - 1;
  }
  return p;
}

// rgan_diffaug_p: `policy` restricted to the groups sample b's gates open, gate[b][g] < (float)*p
// (strict; columns 0, 1, 2 = colour, translation, cutout).  Everything downstream sees that
// mask as the sample's policy, so a closed group takes the same path as a cleared policy bit.
__device__ __forceinline__ int aug_open(const float* __restrict__ gate, const double* __restrict__ prob, int b,
                                        int policy) {
  const float p = (float)prob[0];
  const float* g = gate + 4LL * b;
  return policy & ((g[0] < p ? 1 : 0) | (g[1] < p ? 2 : 0) | (g[2] < p ? 4 : 0));
}

// reduction blocks per sample for `items` work items: ~1024 items (four per thread) each
static inline int aug_blocks(long long items) {
  return (int)std::min<long long>(std::max<long long>((items + 1023) / 1024, 1), 64);
}

}  // namespace rgan
