// Differentiable augmentation of D's inputs (--rgan_diffaug; no reference counterpart: the
// reference trains on the raw batches).  One random colour / translation / cutout transform
// per sample, applied to every image D sees, and its adjoint for the generator's gradient.
//
// For fixed per-sample parameters the transform is affine in the image:
//   col(x)[c,i,j] = con (sat (x[c,i,j] - m_ij) + m_ij - mu) + mu + beta
//   y[c,i,j]      = 0 inside the cutout box or where (i+tx, j+ty) leaves the image,
//                   col(x)[c,i+tx,j+ty] otherwise
// with m_ij the channel mean at a pixel and mu the sample mean.  The adjoint scatters dy back
// through the same move (g), then applies the colour map's linear part, which is symmetric:
//   dx = con (sat g + (1 - sat) mean_c g) + (1 - con) mean_{c,i,j} g.
// Both directions are "one sample sum, then one pass": aug_reduce writes per-block partial
// sums of the sample (of x, or of the scattered g) to the caller's workspace, aug_apply adds
// them in index order (no atomics: two calls give the same bits) and makes the pass.  Without
// the colour bit the pass is a pure move (values copied bit for bit, zeros elsewhere) and the
// reduction is skipped.
//
// Work is split by pixel, not by sample: a work item is VEC consecutive pixels of one row with
// all their channels (the channel mean needs them together), so a 3 x 256 x 256 sample spreads
// over 64 blocks.  VEC = 4 (16-byte loads and stores) needs W % 4 == 0 and 16-byte aligned
// tensors; a sample whose column shift is not a multiple of 4 then loads its sources as
// scalars and still stores 16 bytes.  Other widths run the VEC = 1 instantiation.
#include "augment.h"

#include <climits>

namespace rgan {

// ws[b][blockIdx.x] = this block's share of the sample sum: of x (forward), or of the dy
// positions the adjoint scatters back (not cut out, target inside the image).  Block k sums
// items [k per, (k+1) per) of the sample, each thread its items in order, then block_sum.
template <int VEC, bool GATED>
__global__ __launch_bounds__(256) void aug_reduce(const float* __restrict__ in, const float* __restrict__ u, int C,
                                                  int H, int W, int policy, int adjoint, float* __restrict__ ws,
                                                  const float* __restrict__ gate, const double* __restrict__ prob) {
  __shared__ float red[16];
  const int b = blockIdx.y, nblk = gridDim.x;
  if (GATED) {
    policy = aug_open(gate, prob, b, policy);
    if (!(policy & 1)) return;  // whole block (b is per block): aug_apply moves this sample, ws unread
  }
  const AugParam p = aug_param(u, b, H, W, policy);
  const int items = H * W / VEC;
  const int per = (items + nblk - 1) / nblk;
  const int end = min(items, (int)(blockIdx.x + 1) * per);
  const long long plane = (long long)H * W;
  const float* xb = in + (long long)b * C * plane;
  float acc = 0.f;
  for (int q = blockIdx.x * per + threadIdx.x; q < end; q += blockDim.x) {
    const int pix = q * VEC, i = pix / W, j = pix - i * W;
    bool ok[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) ok[k] = true;
    if (adjoint) {
      const bool row_in = (unsigned)(i + p.tx) < (unsigned)H, row_cut = i >= p.r0 && i <= p.r1;
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        ok[k] = row_in && (unsigned)(j + k + p.ty) < (unsigned)W && !(row_cut && j + k >= p.c0 && j + k <= p.c1);
    }
    for (int c = 0; c < C; ++c) {
      const float* src = xb + c * plane + pix;
      float v[VEC];
      if (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(src);
        v[0] = t.x; v[1 % VEC] = t.y; v[2 % VEC] = t.z; v[3 % VEC] = t.w;
      } else {
        v[0] = src[0];
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc += ok[k] ? v[k] : 0.f;
    }
  }
  const float total = block_sum(acc, red);
  if (threadIdx.x == 0) ws[(long long)b * nblk + blockIdx.x] = total;
}

// One item (VEC pixels x C channels) per thread.  `in` is x (forward) or dy (adjoint); the
// adjoint reads through the opposite shift and tests the cutout box at its SOURCE position
// (the forward's output position).
template <int VEC, bool GATED>
__global__ __launch_bounds__(256) void aug_apply(const float* __restrict__ in, const float* __restrict__ u, int C,
                                                 int H, int W, int policy, int adjoint, int nblk,
                                                 const float* __restrict__ ws, float* __restrict__ out,
                                                 const float* __restrict__ gate, const double* __restrict__ prob) {
  const int b = blockIdx.y;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= H * W / VEC) return;
  if (GATED) policy = aug_open(gate, prob, b, policy);
  const AugParam p = aug_param(u, b, H, W, policy);
  const bool colour = policy & 1;
  const long long plane = (long long)H * W;
  float mean = 0.f;  // mu of x (forward) / of the scattered g (adjoint)
  if (colour) {
    double t = 0.0;
    for (int k = 0; k < nblk; ++k) t += (double)ws[(long long)b * nblk + k];
    mean = (float)(t / ((double)C * (double)plane));
  }
  const int si = adjoint ? -p.tx : p.tx, sj = adjoint ? -p.ty : p.ty;
  const int pix = q * VEC, i = pix / W, j = pix - i * W;
  const int srow = i + si;
  const bool row_in = (unsigned)srow < (unsigned)H;
  const int crow = adjoint ? srow : i;
  const bool row_cut = crow >= p.r0 && crow <= p.r1;
  bool ok[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const int scol = j + k + sj, ccol = adjoint ? scol : j + k;
    ok[k] = row_in && (unsigned)scol < (unsigned)W && !(row_cut && ccol >= p.c0 && ccol <= p.c1);
  }
  const float* xb = in + (long long)b * C * plane;
  float* yb = out + (long long)b * C * plane + pix;
  // a shift by a multiple of 4 keeps the four sources one aligned quad, inside or outside the row
  const bool wide = VEC == 4 && (sj & 3) == 0;

  auto load = [&](int c, float (&v)[VEC]) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = 0.f;
    if (!row_in) return;
    const float* row = xb + c * plane + (long long)srow * W;
    if (VEC == 4 && wide) {
      if ((unsigned)(j + sj) < (unsigned)W) {
        const float4 t = *reinterpret_cast<const float4*>(row + j + sj);
        v[0] = ok[0] ? t.x : 0.f; v[1 % VEC] = ok[1 % VEC] ? t.y : 0.f;
        v[2 % VEC] = ok[2 % VEC] ? t.z : 0.f; v[3 % VEC] = ok[3 % VEC] ? t.w : 0.f;
      }
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        if (ok[k]) v[k] = row[j + k + sj];
    }
  };
  auto store = [&](int c, const float (&v)[VEC]) {
    float* dst = yb + c * plane;
    if (VEC == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1 % VEC], v[2 % VEC], v[3 % VEC]);
    else dst[0] = v[0];
  };
  // v = the moved value (0 where nothing arrives), m = its channel mean at the pixel
  auto colour_map = [&](float v, float m, bool keep) {
    if (adjoint) return p.con * (p.sat * v + (1.f - p.sat) * m) + (1.f - p.con) * mean;
    return keep ? p.con * (p.sat * (v - m) + m - mean) + mean + p.beta : 0.f;
  };

  if (!colour) {  // pure move
    for (int c = 0; c < C; ++c) {
      float v[VEC];
      load(c, v);
      store(c, v);
    }
    return;
  }
  const float inv_c = 1.f / (float)C;
  float m[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) m[k] = 0.f;
  if (C <= 4) {  // the image layers' case: every channel stays in registers
    float v[4][VEC];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < C) {
        load(c, v[c]);
#pragma unroll
        for (int k = 0; k < VEC; ++k) m[k] += v[c][k];
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < C) {
        float o[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) o[k] = colour_map(v[c][k], m[k] * inv_c, ok[k]);
        store(c, o);
      }
    }
    return;
  }
  for (int c = 0; c < C; ++c) {  // wider inputs: a second read (from cache) instead of registers
    float v[VEC];
    load(c, v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) m[k] += v[k];
  }
  for (int c = 0; c < C; ++c) {
    float v[VEC], o[VEC];
    load(c, v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) o[k] = colour_map(v[k], m[k] * inv_c, ok[k]);
    store(c, o);
  }
}

}  // namespace rgan

using namespace rgan;

extern "C" size_t rgan_diffaug_workspace(int batch, int channels, int h, int w) {
  if (batch <= 0 || channels <= 0 || h <= 0 || w <= 0) return 0;
  return (size_t)batch * (size_t)aug_blocks((long long)h * w);  // the VEC = 1 split: the larger one
}

// Both entry points: gate == nullptr runs the ungated instantiations (rgan_diffaug), whose
// instructions are the ones they were before the gate existed (gate and p are the kernels' last
// arguments, so even the argument offsets are).
static int aug_launch(const float* x, const float* u, const float* gate, const double* p, int batch, int channels,
                      int h, int w, int policy, int adjoint, float* ws, float* y, void* stream) {
  RGAN_REQUIRE(x && u && ws && y && x != y);
  RGAN_REQUIRE(batch > 0 && channels > 0 && h > 0 && w > 0 && policy >= 0 && policy <= 7);
  // (two steps: the product of three ints near 2^31 would overflow 64 bits)
  RGAN_REQUIRE(batch <= 65535 && (long long)channels * h <= INT_MAX && (long long)channels * h * w <= INT_MAX);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = w % 4 == 0 && ((uintptr_t)x | (uintptr_t)y) % 16 == 0;
  const int items = h * w / (vec ? 4 : 1);
  const int nblk = aug_blocks(items);
  adjoint = adjoint != 0;
  if (policy & 1) {
    const dim3 grid(nblk, batch);
    if (gate) {
      if (vec) aug_reduce<4, true><<<grid, 256, 0, s>>>(x, u, channels, h, w, policy, adjoint, ws, gate, p);
      else aug_reduce<1, true><<<grid, 256, 0, s>>>(x, u, channels, h, w, policy, adjoint, ws, gate, p);
    } else {
      if (vec) aug_reduce<4, false><<<grid, 256, 0, s>>>(x, u, channels, h, w, policy, adjoint, ws, gate, p);
      else aug_reduce<1, false><<<grid, 256, 0, s>>>(x, u, channels, h, w, policy, adjoint, ws, gate, p);
    }
    RGAN_CHECK_LAUNCH();
  }
  const int threads = items >= 4096 ? 256 : 64;  // small images: more, smaller blocks
  const dim3 grid(ceil_div(items, threads), batch);
  if (gate) {
    if (vec) aug_apply<4, true><<<grid, threads, 0, s>>>(x, u, channels, h, w, policy, adjoint, nblk, ws, y, gate, p);
    else aug_apply<1, true><<<grid, threads, 0, s>>>(x, u, channels, h, w, policy, adjoint, nblk, ws, y, gate, p);
  } else {
    if (vec) aug_apply<4, false><<<grid, threads, 0, s>>>(x, u, channels, h, w, policy, adjoint, nblk, ws, y, gate, p);
    else aug_apply<1, false><<<grid, threads, 0, s>>>(x, u, channels, h, w, policy, adjoint, nblk, ws, y, gate, p);
  }
  RGAN_CHECK_LAUNCH();
  return 0;
}

extern "C" int rgan_diffaug(const float* x, const float* u, int batch, int channels, int h, int w, int policy,
                            int adjoint, float* ws, float* y, void* stream) {
  return aug_launch(x, u, nullptr, nullptr, batch, channels, h, w, policy, adjoint, ws, y, stream);
}

extern "C" int rgan_diffaug_p(const float* x, const float* u, const float* gate, const double* p, int batch,
                              int channels, int h, int w, int policy, int adjoint, float* ws, float* y,
                              void* stream) {
  RGAN_REQUIRE(gate && p);
  return aug_launch(x, u, gate, p, batch, channels, h, w, policy, adjoint, ws, y, stream);
}
