// Geometric groups of --rgan_diffaug (x-flip, quarter turns, warp; no reference counterpart),
// composed with the colour / translation / cutout groups of csrc/augment.hip:
//   y = cutout( translate( Warp( Rot90^k( Flip( col(x) ) ) ) ) )
// One more row of uniforms per sample, v[b][8]: v0 flip, v1 quarter turns, v2 zoom, v3 angle,
// v4..v6 the gates of the three groups (read only when gating is on), v7 reserved.
//
// Flip and the quarter turns are symmetries of the pixel lattice, so they fold into one signed
// permutation M and an offset per sample; the warp multiplies it by a rotation and a zoom:
//   source of the moved position p = (i + tx, j + ty):  centre + A (p - centre),  A = M Rot(theta) / s.
// A sample without an open warp group (or whose warp is the identity, s = 1 and theta = 0) takes
// the integer path: values are copied bit for bit, and with the colour bit the arithmetic is that
// of csrc/augment.hip's aug_apply.  A warped sample gathers four bilinear taps of the raw x per
// value (zero outside the image) and applies the colour map, which is affine, afterwards:
//   y_c = con (sat (X_c - M) + M) + ((1 - con) mu + beta) Wsum,
// X_c the gathered channel, M its channel mean, Wsum the sum of the in-image tap weights.
//
// The adjoint is the exact transpose, written as a gather: the outputs that read source pixel q
// with a non-zero weight lie in A^-1 (q + (-1, 1)^2), a rotated square of side 2 s <= 2 2^(1/4)
// whose bounding box holds at most 4 integers per axis, so dx[q] is a fixed-order sum over 4 x 4
// candidate outputs, each weight recomputed exactly as the forward computes it.  The sample sum
// the colour map's adjoint needs equals sum_a g[a] Wsum(a), a gather over dy as well.  No
// atomics anywhere: two calls give the same bits.
//
// Coordinates are computed in double (one sincos and one exp2 per block, kept in LDS; two FMAs
// per coordinate and pixel): in float a coordinate near 256 carries 3e-5 of rounding, which a
// unit slope of the image turns into the same error of the value.
//
// Work split, reduction and stores are csrc/augment.hip's: an item is VEC consecutive pixels of
// a row with all their channels, VEC = 4 (16-byte stores) when W % 4 == 0 and the tensors are
// aligned; source taps are scalar loads.
#include "augment.h"

#include <climits>

namespace rgan {

struct GeoParam {
  AugParam a;
  int policy;                  // the sample's open groups
  int warp;                    // 1: bilinear path
  int m00, m01, m10, m11;      // M: x index = o + M p (flip after k quarter turns)
  int orow, ocol, prow, pcol;  // offsets of M and of its inverse (p = po + M^t q)
  double A00, A01, A10, A11;   // x - centre = A (p - centre)
  double B00, B01, B10, B11;   // p - centre = B (x - centre), B = A^-1
  double ext;                  // half extent per axis of B (-1, 1)^2
  double ci, cj;
};

// Sample b's parameters (one thread per block computes them).  With gating, a group is open
// iff its gate is below (float)*p, strict: colour / translation / cutout from gate[b][0..2] as
// aug_open has it, x-flip / quarter turns / warp from v[b][4..6].
__device__ void geo_param(GeoParam& g, const float* __restrict__ u, const float* __restrict__ v,
                          const float* __restrict__ gate, const double* __restrict__ prob, int b, int H, int W,
                          int policy) {
  const float* r = v + 8LL * b;
  if (gate) {
    const float p = (float)prob[0];
    policy = aug_open(gate, prob, b, policy & 7) |
             (policy & ((r[4] < p ? 8 : 0) | (r[5] < p ? 16 : 0) | (r[6] < p ? 32 : 0)));
  }
  g.policy = policy;
  g.a = aug_param(u, b, H, W, policy);
  const int fl = (policy & 8) && r[0] >= 0.5f ? -1 : 1;
  const int k = (policy & 16) ? aug_pick(r[1], 4) : 0;
  // torch.rot90(z, 1, (2, 3))[i, j] = z[j, N - 1 - i]: about the centre, (a, b) -> (b, -a)
  int r00 = 1, r01 = 0, r10 = 0, r11 = 1;
  if (k == 1) { r00 = 0; r01 = 1; r10 = -1; r11 = 0; }
  if (k == 2) { r00 = -1; r11 = -1; }
  if (k == 3) { r00 = 0; r01 = -1; r10 = 1; r11 = 0; }
  g.m00 = r00; g.m01 = r01; g.m10 = fl * r10; g.m11 = fl * r11;
  // centre - M centre, an integer: odd quarter turns come with H == W (checked on the host)
  g.orow = ((H - 1) * (1 - g.m00) - g.m01 * (W - 1)) / 2;
  g.ocol = ((W - 1) * (1 - g.m11) - g.m10 * (H - 1)) / 2;
  g.prow = ((H - 1) * (1 - g.m00) - g.m10 * (W - 1)) / 2;
  g.pcol = ((W - 1) * (1 - g.m11) - g.m01 * (H - 1)) / 2;
  g.ci = 0.5 * (double)(H - 1);
  g.cj = 0.5 * (double)(W - 1);
  g.warp = 0;
  g.A00 = g.A01 = g.A10 = g.A11 = g.B00 = g.B01 = g.B10 = g.B11 = g.ext = 0.0;
  if (policy & 32) {
    const double s = exp2(((double)r[2] - 0.5) * 0.5);
    const double theta = (2.0 * (double)r[3] - 1.0) * 3.14159265358979323846;
    if (!(s == 1.0 && theta == 0.0)) {  // (the identity stays on the integer path)
      double sn, cs;
      sincos(theta, &sn, &cs);
      const double is = 1.0 / s;
      const double P00 = cs * is, P01 = sn * is, P10 = -sn * is, P11 = cs * is;  // Rot(theta) / s
      g.A00 = g.m00 * P00 + g.m01 * P10; g.A01 = g.m00 * P01 + g.m01 * P11;
      g.A10 = g.m10 * P00 + g.m11 * P10; g.A11 = g.m10 * P01 + g.m11 * P11;
      const double Q00 = cs * s, Q01 = -sn * s, Q10 = sn * s, Q11 = cs * s;  // s Rot(-theta)
      g.B00 = Q00 * g.m00 + Q01 * g.m01; g.B01 = Q00 * g.m10 + Q01 * g.m11;  // times M^t
      g.B10 = Q10 * g.m00 + Q11 * g.m01; g.B11 = Q10 * g.m10 + Q11 * g.m11;
      g.ext = s * (fabs(cs) + fabs(sn)) + 1e-6;
      g.warp = 1;
    }
  }
}

// The four bilinear taps of the moved position (pr, pc): rows r0, r0 + 1, columns c0, c0 + 1;
// a weight is 0 where its row / column lies outside the image, so a non-zero weight product
// names a tap that may be loaded.  Whatever v held (nan included), the coordinate is clamped
// before it becomes an integer.
struct GeoTaps {
  int r0, c0;
  float wr0, wr1, wc0, wc1;
};

__device__ __forceinline__ GeoTaps geo_taps(const GeoParam& g, int pr, int pc, int H, int W) {
  const double di = (double)pr - g.ci, dj = (double)pc - g.cj;
  double r = fma(g.A01, dj, fma(g.A00, di, g.ci));
  double c = fma(g.A11, dj, fma(g.A10, di, g.cj));
  r = fmin(fmax(r, -2.0), (double)H + 1.0);
  c = fmin(fmax(c, -2.0), (double)W + 1.0);
  const double fr0 = floor(r), fc0 = floor(c);
  const double fr = r - fr0, fc = c - fc0;
  GeoTaps t;
  t.r0 = (int)fr0;
  t.c0 = (int)fc0;
  t.wr0 = (unsigned)t.r0 < (unsigned)H ? (float)(1.0 - fr) : 0.f;
  t.wr1 = (unsigned)(t.r0 + 1) < (unsigned)H ? (float)fr : 0.f;
  t.wc0 = (unsigned)t.c0 < (unsigned)W ? (float)(1.0 - fc) : 0.f;
  t.wc1 = (unsigned)(t.c0 + 1) < (unsigned)W ? (float)fc : 0.f;
  return t;
}

__device__ __forceinline__ float geo_wsum(const GeoTaps& t) { return (t.wr0 + t.wr1) * (t.wc0 + t.wc1); }

__device__ __forceinline__ bool geo_cut(const AugParam& p, int i, int j) {
  return i >= p.r0 && i <= p.r1 && j >= p.c0 && j <= p.c1;
}

// Channels c0 .. c0 + 3 (those below C) of the moved / gathered value at pixel (i, j), before
// the colour map: of x at output (i, j) (forward), or of dy scattered back to source (i, j)
// (adjoint).  keep: the forward's output receives a value (not cut out, moved position inside
// the image); wsum: the forward's tap weight sum there.  xb: the sample's first element.
__device__ __forceinline__ void geo_fetch(const GeoParam& g, int adjoint, const float* __restrict__ xb, int C, int H,
                                          int W, long long plane, int i, int j, int c0, float (&val)[4], bool& keep,
                                          float& wsum) {
  const AugParam& p = g.a;
#pragma unroll
  for (int c = 0; c < 4; ++c) val[c] = 0.f;
  wsum = 1.f;
  if (!g.warp) {  // integer path: one source, copied
    int si, sj;
    if (!adjoint) {
      const int pr = i + p.tx, pc = j + p.ty;
      si = g.orow + g.m00 * pr + g.m01 * pc;
      sj = g.ocol + g.m10 * pr + g.m11 * pc;
      keep = (unsigned)pr < (unsigned)H && (unsigned)pc < (unsigned)W && !geo_cut(p, i, j);
    } else {
      si = g.prow + g.m00 * i + g.m10 * j - p.tx;
      sj = g.pcol + g.m01 * i + g.m11 * j - p.ty;
      keep = !geo_cut(p, si, sj);
    }
    keep = keep && (unsigned)si < (unsigned)H && (unsigned)sj < (unsigned)W;
    if (keep) {
      const float* s = xb + (long long)si * W + sj;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c0 + c < C) val[c] = s[(c0 + c) * plane];
    }
    return;
  }
  if (!adjoint) {
    const int pr = i + p.tx, pc = j + p.ty;
    keep = (unsigned)pr < (unsigned)H && (unsigned)pc < (unsigned)W && !geo_cut(p, i, j);
    if (!keep) {
      wsum = 0.f;
      return;
    }
    const GeoTaps t = geo_taps(g, pr, pc, H, W);
    wsum = geo_wsum(t);
    const bool t00 = t.wr0 != 0.f && t.wc0 != 0.f, t01 = t.wr0 != 0.f && t.wc1 != 0.f;
    const bool t10 = t.wr1 != 0.f && t.wc0 != 0.f, t11 = t.wr1 != 0.f && t.wc1 != 0.f;
    const float* s = xb + (long long)t.r0 * W + t.c0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c0 + c < C) {
        const float* sc = s + (c0 + c) * plane;
        const float v00 = t00 ? sc[0] : 0.f, v01 = t01 ? sc[1] : 0.f;
        const float v10 = t10 ? sc[W] : 0.f, v11 = t11 ? sc[W + 1] : 0.f;
        val[c] = t.wr0 * (t.wc0 * v00 + t.wc1 * v01) + t.wr1 * (t.wc0 * v10 + t.wc1 * v11);
      }
    }
    return;
  }
  // adjoint of the gather, as a gather: the 4 x 4 candidate moved positions around B (q - centre)
  keep = true;
  const double qi = (double)i - g.ci, qj = (double)j - g.cj;
  const double pr_c = fma(g.B01, qj, fma(g.B00, qi, g.ci)), pc_c = fma(g.B11, qj, fma(g.B10, qi, g.cj));
  const int lo_r = (int)ceil(fmin(fmax(pr_c - g.ext, -4.0), (double)H + 4.0));
  const int lo_c = (int)ceil(fmin(fmax(pc_c - g.ext, -4.0), (double)W + 4.0));
  for (int dr = 0; dr < 4; ++dr) {
    const int pr = lo_r + dr, ai = pr - p.tx;
    if ((unsigned)pr >= (unsigned)H || (unsigned)ai >= (unsigned)H) continue;
    for (int dc = 0; dc < 4; ++dc) {
      const int pc = lo_c + dc, aj = pc - p.ty;
      if ((unsigned)pc >= (unsigned)W || (unsigned)aj >= (unsigned)W || geo_cut(p, ai, aj)) continue;
      const GeoTaps t = geo_taps(g, pr, pc, H, W);
      const float wr = i == t.r0 ? t.wr0 : (i == t.r0 + 1 ? t.wr1 : 0.f);
      const float wc = j == t.c0 ? t.wc0 : (j == t.c0 + 1 ? t.wc1 : 0.f);
      const float w = wr * wc;
      if (w != 0.f) {
        const float* s = xb + (long long)ai * W + aj;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c0 + c < C) val[c] = fmaf(w, s[(c0 + c) * plane], val[c]);
      }
    }
  }
}

// ws[b][blockIdx.x] = this block's share of the sample sum, split and ordered as aug_reduce
// has it: of x (forward); of g[a] Wsum(a) over the kept outputs a (adjoint; Wsum = 1 on the
// integer path, where this is aug_reduce's sum).
template <int VEC>
__global__ __launch_bounds__(256) void geo_reduce(const float* __restrict__ in, const float* __restrict__ u,
                                                  const float* __restrict__ v, const float* __restrict__ gate,
                                                  const double* __restrict__ prob, int C, int H, int W, int policy,
                                                  int adjoint, float* __restrict__ ws) {
  __shared__ float red[16];
  __shared__ GeoParam sp;
  const int b = blockIdx.y, nblk = gridDim.x;
  if (threadIdx.x == 0) geo_param(sp, u, v, gate, prob, b, H, W, policy);
  __syncthreads();
  const GeoParam& g = sp;
  if (!(g.policy & 1)) return;  // whole block: geo_apply moves this sample, ws unread
  const AugParam p = g.a;
  const bool weigh = adjoint && g.warp;
  const int items = H * W / VEC;
  const int per = (items + nblk - 1) / nblk;
  const int end = min(items, (int)(blockIdx.x + 1) * per);
  const long long plane = (long long)H * W;
  const float* xb = in + (long long)b * C * plane;
  float acc = 0.f;
  for (int q = blockIdx.x * per + threadIdx.x; q < end; q += blockDim.x) {
    const int pix = q * VEC, i = pix / W, j = pix - i * W;
    bool ok[VEC];
    float wt[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      ok[k] = true;
      wt[k] = 1.f;
    }
    if (adjoint) {
      const bool row_in = (unsigned)(i + p.tx) < (unsigned)H, row_cut = i >= p.r0 && i <= p.r1;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        ok[k] = row_in && (unsigned)(j + k + p.ty) < (unsigned)W && !(row_cut && j + k >= p.c0 && j + k <= p.c1);
        if (weigh && ok[k]) wt[k] = geo_wsum(geo_taps(g, i + p.tx, j + k + p.ty, H, W));
      }
    }
    for (int c = 0; c < C; ++c) {
      const float* src = xb + c * plane + pix;
      float x[VEC];
      if (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(src);
        x[0] = t.x; x[1 % VEC] = t.y; x[2 % VEC] = t.z; x[3 % VEC] = t.w;
      } else {
        x[0] = src[0];
      }
      if (weigh) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc += ok[k] ? x[k] * wt[k] : 0.f;
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc += ok[k] ? x[k] : 0.f;
      }
    }
  }
  const float total = block_sum(acc, red);
  if (threadIdx.x == 0) ws[(long long)b * nblk + blockIdx.x] = total;
}

// One item (VEC pixels x C channels) per thread.  `in` is x (forward) or dy (adjoint).
template <int VEC>
__global__ __launch_bounds__(256) void geo_apply(const float* __restrict__ in, const float* __restrict__ u,
                                                 const float* __restrict__ v, const float* __restrict__ gate,
                                                 const double* __restrict__ prob, int C, int H, int W, int policy,
                                                 int adjoint, int nblk, const float* __restrict__ ws,
                                                 float* __restrict__ out) {
  __shared__ GeoParam sp;
  const int b = blockIdx.y;
  if (threadIdx.x == 0) geo_param(sp, u, v, gate, prob, b, H, W, policy);
  __syncthreads();
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= H * W / VEC) return;
  const GeoParam& g = sp;
  const AugParam p = g.a;
  const bool colour = g.policy & 1, warp = g.warp;
  const long long plane = (long long)H * W;
  float mean = 0.f;  // mu of x (forward) / of the scattered g (adjoint)
  if (colour) {
    double t = 0.0;
    for (int k = 0; k < nblk; ++k) t += (double)ws[(long long)b * nblk + k];
    mean = (float)(t / ((double)C * (double)plane));
  }
  const int pix = q * VEC, i = pix / W, j = pix - i * W;
  const float* xb = in + (long long)b * C * plane;
  float* yb = out + (long long)b * C * plane + pix;

  auto store = [&](int c, const float (&o)[VEC]) {
    float* dst = yb + c * plane;
    if (VEC == 4) *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1 % VEC], o[2 % VEC], o[3 % VEC]);
    else dst[0] = o[0];
  };
  // x = the moved / gathered value (0 where nothing arrives), m = its channel mean at the pixel;
  // the integer path's two expressions are aug_apply's
  auto colour_map = [&](float x, float m, bool keep, float wsum) {
    if (adjoint) return p.con * (p.sat * x + (1.f - p.sat) * m) + (1.f - p.con) * mean;
    if (!warp) return keep ? p.con * (p.sat * (x - m) + m - mean) + mean + p.beta : 0.f;
    return keep ? p.con * (p.sat * (x - m) + m) + ((1.f - p.con) * mean + p.beta) * wsum : 0.f;
  };

  bool keep[VEC];
  float wsum[VEC], m[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) m[k] = 0.f;
  const float inv_c = 1.f / (float)C;
  if (C <= 4) {  // the image layers' case: every channel stays in registers
    float val[VEC][4];
#pragma unroll
    for (int k = 0; k < VEC; ++k) geo_fetch(g, adjoint, xb, C, H, W, plane, i, j + k, 0, val[k], keep[k], wsum[k]);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < C) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) m[k] += val[k][c];
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < C) {
        float o[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) o[k] = colour ? colour_map(val[k][c], m[k] * inv_c, keep[k], wsum[k]) : val[k][c];
        store(c, o);
      }
    }
    return;
  }
  // wider inputs: four channels at a time, a second gather (from cache) instead of registers
  if (colour) {
    for (int c0 = 0; c0 < C; c0 += 4) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float val[4];
        geo_fetch(g, adjoint, xb, C, H, W, plane, i, j + k, c0, val, keep[k], wsum[k]);
#pragma unroll
        for (int c = 0; c < 4; ++c) m[k] += val[c];  // (0 for the channels past C)
      }
    }
  }
  for (int c0 = 0; c0 < C; c0 += 4) {
    float val[VEC][4];
#pragma unroll
    for (int k = 0; k < VEC; ++k) geo_fetch(g, adjoint, xb, C, H, W, plane, i, j + k, c0, val[k], keep[k], wsum[k]);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c0 + c < C) {
        float o[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) o[k] = colour ? colour_map(val[k][c], m[k] * inv_c, keep[k], wsum[k]) : val[k][c];
        store(c0 + c, o);
      }
    }
  }
}

}  // namespace rgan

using namespace rgan;

extern "C" size_t rgan_diffaug_geo_workspace(int batch, int channels, int h, int w) {
  return rgan_diffaug_workspace(batch, channels, h, w);
}

extern "C" int rgan_diffaug_geo(const float* x, const float* u, const float* v, const float* gate, const double* p,
                                int batch, int channels, int h, int w, int policy, int adjoint, float* ws, float* y,
                                void* stream) {
  RGAN_REQUIRE((gate == nullptr) == (p == nullptr));
  RGAN_REQUIRE(policy >= 0 && policy <= 63);
  if (!(policy & 56))  // no geometric group: the kernels of csrc/augment.hip
    return gate ? rgan_diffaug_p(x, u, gate, p, batch, channels, h, w, policy, adjoint, ws, y, stream)
                : rgan_diffaug(x, u, batch, channels, h, w, policy, adjoint, ws, y, stream);
  RGAN_REQUIRE(x && u && v && ws && y && x != y);
  RGAN_REQUIRE(batch > 0 && channels > 0 && h > 0 && w > 0);
  // (two steps: the product of three ints near 2^31 would overflow 64 bits)
  RGAN_REQUIRE(batch <= 65535 && (long long)channels * h <= INT_MAX && (long long)channels * h * w <= INT_MAX);
  RGAN_REQUIRE(!(policy & 16) || h == w);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = w % 4 == 0 && ((uintptr_t)x | (uintptr_t)y) % 16 == 0;
  const int items = h * w / (vec ? 4 : 1);
  const int nblk = aug_blocks(items);
  adjoint = adjoint != 0;
  if (policy & 1) {
    const dim3 grid(nblk, batch);
    if (vec) geo_reduce<4><<<grid, 256, 0, s>>>(x, u, v, gate, p, channels, h, w, policy, adjoint, ws);
    else geo_reduce<1><<<grid, 256, 0, s>>>(x, u, v, gate, p, channels, h, w, policy, adjoint, ws);
    RGAN_CHECK_LAUNCH();
  }
  const int threads = items >= 4096 ? 256 : 64;  // small images: more, smaller blocks
  const dim3 grid(ceil_div(items, threads), batch);
  if (vec) geo_apply<4><<<grid, threads, 0, s>>>(x, u, v, gate, p, channels, h, w, policy, adjoint, nblk, ws, y);
  else geo_apply<1><<<grid, threads, 0, s>>>(x, u, v, gate, p, channels, h, w, policy, adjoint, nblk, ws, y);
  RGAN_CHECK_LAUNCH();
  return 0;
}
