// The kernels for layers too narrow for the implicit GEMM -- the one-output dense layer and the
// narrow-channel convolutions -- with the pack of the narrow ConvT weights and their launchers.
#include "conv_plan.h"

namespace rgan {

// ---------------------------------------------------------------- one-output dense layer
// D's closing Conv2d(C, 1, k, 1, 0) over a k x k map (GLI:455, GLI:306) covers the whole
// map: per sample a dot product of C*k*k inputs with the single filter.  As an implicit GEMM
// it is N = 1 (one 32-wide tile column, 1/32 used, split-K 256 ways); here:
//   fwd   one block per sample, y[b] = act(wsc * <x[b], W> + bias)  (fixed-order block sum)
//   dgrad dx[b][e] = (dy[b] * W[e]) * wsc                            (elementwise, NHWC stores)
//   wgrad dW[e] = sum_b dy[b] * x[b][e], b in order                  (thread per filter tap)
// e runs over (h, w, c) with c fastest, so NHWC activations are read/written coalesced; fwd
// and dgrad read the filter packed in the same order (the conv forward pack, [1][(kh,kw,ci)]),
// wgrad writes it in torch order c*k*k + h*k + w.  (DenseArgs: conv_plan.h.)
__device__ __forceinline__ long long dense_x_off(const DenseArgs& a, int e, int& widx) {
  const uint32_t hw = a.fc.div(e);
  const int c = e - (int)(hw * a.fc.d);
  const uint32_t h = a.fw.div(hw);
  const int w = (int)(hw - h * a.fw.d);
  widx = c * a.HW + (int)hw;
  return (long long)c * a.xsc + (long long)h * a.xsh + (long long)w * a.xsw;
}

// VEC (host-checked: channel stride 1, C % 4 == 0, 16-B aligned rows): thread items are
// channel quads, one float4 of activations + 4 filter taps.
// VEC (host-checked: channel stride 1, C % 4 == 0, 16-B aligned rows): thread items are
// channel quads, one float4 of activations and one of packed filter.
template <bool VEC>
__global__ __launch_bounds__(1024) void dense1_fwd(DenseArgs a) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  const float* xb = a.x + (long long)b * a.xsb;
  float acc = 0.f;
  if constexpr (VEC) {
#pragma unroll 8
    for (int e = 4 * threadIdx.x; e < a.E; e += 4 * 1024) {
      int wi;
      const float4 xv = *reinterpret_cast<const float4*>(xb + dense_x_off(a, e, wi));
      const float4 wv = *reinterpret_cast<const float4*>(a.w + e);
      acc = fmaf(xv.x, wv.x, acc);
      acc = fmaf(xv.y, wv.y, acc);
      acc = fmaf(xv.z, wv.z, acc);
      acc = fmaf(xv.w, wv.w, acc);
    }
  } else {
#pragma unroll 8
    for (int e = threadIdx.x; e < a.E; e += 1024) {
      int wi;
      const long long xo = dense_x_off(a, e, wi);
      acc = fmaf(xb[xo], a.w[e], acc);
    }
  }
  const float t = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const float wsc = a.wscale ? a.wscale[0] : 1.f;
    const float v = t * wsc + (a.bias ? a.bias[0] : 0.f);
    a.y[(long long)b * a.ysb] = act_fwd(v, a.act, a.alpha);
  }
}

// fe = E / (VEC ? 4 : 1): item -> (b, e)
template <bool VEC>
__global__ __launch_bounds__(256) void dense1_dgrad(DenseArgs a, FastDiv fe) {
  const uint32_t total = (uint32_t)a.B * fe.d;
  const float wsc = a.wscale ? a.wscale[0] : 1.f;
  for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
    const uint32_t b = fe.div(idx);
    const int e = (int)(idx - b * fe.d) * (VEC ? 4 : 1);
    int wi;
    const long long xo = dense_x_off(a, e, wi);
    const float g = a.y[(long long)b * a.ysb];
    float* o = a.out + (long long)b * a.xsb + xo;
    if constexpr (VEC) {
      const float4 wv = *reinterpret_cast<const float4*>(a.w + e);
      *reinterpret_cast<float4*>(o) = make_float4((g * wv.x) * wsc, (g * wv.y) * wsc, (g * wv.z) * wsc,
                                                  (g * wv.w) * wsc);
    } else {
      *o = (g * a.w[e]) * wsc;
    }
  }
}

__global__ __launch_bounds__(256) void dense1_wgrad(DenseArgs a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.E) return;
  int wi;
  const long long xo = dense_x_off(a, e, wi);
  float acc = 0.f;
#pragma unroll 16
  for (int b = 0; b < a.B; ++b) acc = fmaf(a.y[(long long)b * a.ysb], a.x[(long long)b * a.xsb + xo], acc);
  a.out[wi] = a.accum ? a.out[wi] + acc : acc;
}

// ---------------------------------------------------------------- narrow convolutions
// The image layers do not fit the pipelined GEMM: N <= 4 wastes >= 88% of a 32-wide MFMA
// tile, and K = 16*CI <= 64 is one or two BK tiles around a full prologue and epilogue:
//   convt2_narrow_mfma   k4 s2 p1 ConvTranspose2d (and the Conv2d dgrad of the same shape)
//                        with <= 4 output channels: G's image layer (GLI:448) and D's image
//                        gradient (the backward of GLI:410 into G), on 4x4x1 MFMA blocks.
//   conv_narrow_in_mfma  Conv2d with <= 4 input channels and a 4x4 kernel: D's image layer
//                        (GLI:410) as a single-pass MFMA tile (below).

// Conv2d with a 4x4 kernel and CI <= 4 input channels (D's image layer, GLI:410) as ONE MFMA
// GEMM tile pass: M = output pixels, N = Cout, K = 16*CI (16..64).  K is too short for the
// pipelined GEMM (one or two BK tiles around a full prologue/epilogue, and a per-element
// im2col index decomposition in every tile), so a block builds its whole 128 x K im2col
// tile once (per-row pixel decomposition, per-k (ci, kh, kw) from bit fields), stages the
// 128 x K weight tile straight from torch layout ([co][ci][kh][kw] = [n][k], k-contiguous),
// and runs K/2 MFMA steps per accumulator from k-contiguous LDS rows (row stride K+4 dwords,
// an odd number of 16-B slots: conflict-free ds_read_b128; lane half h takes k in
// [h K/2, (h+1) K/2)).  Persistent over M tiles (next tile's im2col loads in flight during
// this tile's MFMAs); the product is formed transposed (rows = channels) so the NHWC
// epilogue is one float4 store per 4 channels.  Measured (C2 D image layer, 64x3x128^2 ->
// 128 ch): 100 us as one VALU thread per pixel, 76 us here; without the stores 53 us --
// fp32 MFMA and VALU share one issue pipe on gfx950, so the im2col/epilogue VALU is paid
// in MFMA time.
template <int CI>
__global__ __launch_bounds__(256, 2) void conv_narrow_in_mfma(NarrowArgs a) {
  constexpr int K = CI * 16, KH2 = K / 2, LD = K + 4;
  __shared__ __attribute__((aligned(16))) float As[128 * LD];
  __shared__ __attribute__((aligned(16))) float Bs[128 * LD];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l32 = lane & 31, lk = lane >> 5;
  const int wm = (wid >> 1) * 64, wn = (wid & 1) * 64;
  __shared__ long long moff[128];
  const int HWo = a.Ho * a.Wo, M = a.B * HWo, tiles = (M + 127) / 128;
  const int n0 = blockIdx.y * 128;
  {
    // all K/2 weight loads in flight before the first LDS store (a rolled loop would wait
    // on each load in turn: ~24 serialised L2 round trips per block)
    float wv[K / 2];
#pragma unroll
    for (int j = 0; j < K / 2; ++j) {
      const int e = tid + 256 * j, r = e / K, k = e - r * K, n = n0 + r;
      wv[j] = n < a.Cout ? a.w[(size_t)n * K + k] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < K / 2; ++j) {
      const int e = tid + 256 * j, r = e / K, k = e - r * K;
      Bs[r * LD + k] = wv[j];
    }
  }
  // im2col of one tile into registers: thread = (row tid/2, half tid%2 of the K columns)
  const int row = tid >> 1, half = tid & 1;
  float av[KH2];
  auto gather = [&](int m0) {
    const int m = m0 + row;
    if (m < M) {
      const int b = m / HWo, rem = m - b * HWo, oi = rem / a.Wo, oj = rem - oi * a.Wo;
      const int ih0 = oi * a.stride - a.pad, iw0 = oj * a.stride - a.pad;
      const float* xb = a.x + (long long)b * a.xsb;
#pragma unroll
      for (int kk = 0; kk < KH2; ++kk) {
        const int k = half * KH2 + kk, ci = k >> 4, ih = ih0 + ((k >> 2) & 3), iw = iw0 + (k & 3);
        av[kk] = ((unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
                     ? xb[(long long)ci * a.xsc + (long long)ih * a.xsh + (long long)iw * a.xsw]
                     : 0.f;
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < KH2; ++kk) av[kk] = 0.f;
    }
  };
  const float wsc = a.wscale ? a.wscale[0] : 1.f;
  const float* Ar = As + (wm + l32) * LD + lk * KH2;
  const float* Br = Bs + (wn + l32) * LD + lk * KH2;
  // persistent over M tiles: the next tile's im2col loads are in flight during this tile's
  // MFMAs and stores (one block per tile spent most of its life waiting on them)
  int t = blockIdx.x;
  if (t < tiles) gather(t * 128);
  for (; t < tiles; t += gridDim.x) {
    const int m0 = t * 128;
#pragma unroll
    for (int kk = 0; kk < KH2; ++kk) As[row * LD + half * KH2 + kk] = av[kk];
    if (tid < 128) {
      const int m = m0 + tid;
      long long o = -1;
      if (m < M) {
        const int b = m / HWo, rem = m - b * HWo, oi = rem / a.Wo, oj = rem - oi * a.Wo;
        o = (long long)b * a.ysb + (long long)oi * a.ysh + (long long)oj * a.ysw;
      }
      moff[tid] = o;
    }
    __syncthreads();
    if (t + (int)gridDim.x < tiles) gather((t + gridDim.x) * 128);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // transposed product: rows = output channels (A = weights), columns = pixels (B =
    // im2col), so each lane holds 4 consecutive channels of one pixel per register quad
    // and the NHWC store is one float4
#pragma unroll
    for (int q = 0; q < KH2 / 4; ++q) {
      float4 a4[2], b4[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        a4[u] = *reinterpret_cast<const float4*>(Ar + 32 * u * LD + 4 * q);
        b4[u] = *reinterpret_cast<const float4*>(Br + 32 * u * LD + 4 * q);
      }
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b4[j][s4], a4[i][s4], acc[i][j], 0, 0, 0);
    }
    const bool vec4 = a.ysc == 1 && (a.Cout & 3) == 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long long o = moff[wm + 32 * i + l32];  // this lane's pixel
      if (o < 0) continue;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int cb = n0 + wn + 32 * j + 8 * g + 4 * lk;  // channels cb .. cb+3
          if (cb >= a.Cout) continue;
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[e] = act_fwd(acc[i][j][4 * g + e] * wsc + (a.bias && cb + e < a.Cout ? a.bias[cb + e] : 0.f), a.act,
                           a.alpha);
          if (vec4) {
            *reinterpret_cast<float4*>(a.y + o + cb) = make_float4(v[0], v[1], v[2], v[3]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (cb + e < a.Cout) a.y[o + (long long)(cb + e) * a.ysc] = v[e];
          }
        }
    }
    __syncthreads();  // As / moff are rewritten for the next tile
  }
}

// Conv2d 3x3 stride 1 with NC <= 4 output channels over an NHWC input of C channels (C a power
// of two, 4 <= C <= 256): arch 1's image layer (GLI:222-223) and, reading the kernel transposed
// and flipped, the data gradient of arch 1's 3-channel input layer (GLI:202, the WGAN-GP input
// gradient).  As an implicit GEMM (N = NC) every MFMA would be >= 7/8 padding.  Here L = C / 4
// lanes share a pixel, lane l owning channels 4 l .. 4 l + 3: it holds their 9 x 4 x NC weights
// in registers for the whole wave, so a pixel costs each lane 9 float4 loads (the L lanes of a
// tap read one contiguous C * 4-byte run) and 36 NC FMAs, after which a log2(L)-step xor
// butterfly adds the lanes (a + b == b + a: every lane of a pixel holds the same sums) and lane
// o mod L stores output o.  A wave walks `steps` groups of 64 / L pixels, two groups' loads in
// flight together; waves are independent (no LDS, no barrier).  Round 6: a thread
// per (pixel, quarter of the channels) ran 9 x C / 16 dependent load -> FMA steps at C4 (C =
// 128), latency-bound at 14.1 us per call whatever the pixels per thread.
template <int NC>
__global__ __launch_bounds__(64 * N3_WAVES) void conv3_narrow_out(NarrowArgs a, int steps) {
  extern __shared__ float wl[];  // [L][9][4][NC]: lane sl's weights contiguous
  const int C = a.C, L = C >> 2, PW = 64 / L;
  const int lc = __builtin_ctz(C);  // C is a power of two
  for (int i = threadIdx.x; i < 9 * C * NC; i += 64 * N3_WAVES) {
    const int o = i % NC, e = i / NC, c = e & (C - 1), t = e >> lc;  // reads: o fastest, then channel
    wl[(((c >> 2) * 9 + t) * 4 + (c & 3)) * NC + o] =
        a.w[o * (int)a.w_sn + c * (int)a.w_sc + (a.w_flip ? 8 - t : t)];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, sl = lane & (L - 1);
  const int HW = a.Ho * a.Wo, P = a.B * HW;  // < 2^31 (plan)
  const int pix0 = (blockIdx.x * N3_WAVES + (threadIdx.x >> 6)) * steps * PW;
  if (pix0 >= P) return;  // whole wave: no barrier below
  float w[9][4][NC];
  {
    const float* src = wl + sl * 36 * NC;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int o = 0; o < NC; ++o) w[t][k][o] = src[(t * 4 + k) * NC + o];
  }
  const float wsc = a.wscale ? a.wscale[0] : 1.f;
  float bo[NC];
#pragma unroll
  for (int o = 0; o < NC; ++o) bo[o] = a.bias ? a.bias[o] : 0.f;
  // x through a buffer descriptor: a tap outside the image (or a pixel past P) gets an offset
  // past the extent and the load returns zeros -- every load unconditional, no branch (a
  // conditional load is compiled into a branch that waits for it: one load in flight)
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, a.x_bytes, 0x00020000);
  const int xsb = 4 * (int)a.xsb, xsh = 4 * (int)a.xsh, xsw = 4 * (int)a.xsw;  // bytes
  // the lane's pixel (b, oh, ow), advanced by PW per group without a division
  int pix = pix0 + lane / L, b = pix / HW, r = pix - b * HW, oh = r / a.Wo, ow = r - oh * a.Wo;
  auto advance = [&]() {
    pix += PW;
    ow += PW;
    while (ow >= a.Wo) {
      ow -= a.Wo;
      if (++oh == a.Ho) { oh = 0; ++b; }
    }
  };
  auto load = [&](u32x4 (&xv)[9]) {
    const int base = b * xsb + (oh - a.pad) * xsh + (ow - a.pad) * xsw + 16 * sl;
    const bool in = pix < P;
    bool rok[3], cok[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      rok[k] = in & ((unsigned)(oh + k - a.pad) < (unsigned)a.H);
      cok[k] = (unsigned)(ow + k - a.pad) < (unsigned)a.W;
    }
#pragma unroll
    for (int t = 0; t < 9; ++t)
      xv[t] = __builtin_amdgcn_raw_buffer_load_b128(
          xr, (rok[t / 3] & cok[t % 3]) ? base + (t / 3) * xsh + (t % 3) * xsw : 0x7ffffff0, 0, 0);
  };
  auto finish = [&](const u32x4 (&xv)[9], int pb, int ob, int ohb, int owb) {
    float acc[NC];
#pragma unroll
    for (int o = 0; o < NC; ++o) acc[o] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float x0 = __uint_as_float(xv[t].x), x1 = __uint_as_float(xv[t].y), x2 = __uint_as_float(xv[t].z),
                  x3 = __uint_as_float(xv[t].w);
#pragma unroll
      for (int o = 0; o < NC; ++o) acc[o] += x0 * w[t][0][o] + x1 * w[t][1][o] + x2 * w[t][2][o] + x3 * w[t][3][o];
    }
    for (int m = 1; m < L; m <<= 1)
#pragma unroll
      for (int o = 0; o < NC; ++o) acc[o] += __shfl_xor(acc[o], m);
    if (pb >= P) return;
    float* yp = a.y + ob * a.ysb + (long long)ohb * a.ysh + (long long)owb * a.ysw;
    if (L >= NC) {  // lane o stores output o: one activation per lane
      if (sl < NC) {
        float v = acc[0], bb = bo[0];
#pragma unroll
        for (int o = 1; o < NC; ++o) {
          v = sl == o ? acc[o] : v;
          bb = sl == o ? bo[o] : bb;
        }
        yp[(long long)sl * a.ysc] = act_fwd(v * wsc + bb, a.act, a.alpha);
      }
    } else {
#pragma unroll
      for (int o = 0; o < NC; ++o)
        if ((o & (L - 1)) == sl) yp[(long long)o * a.ysc] = act_fwd(acc[o] * wsc + bo[o], a.act, a.alpha);
    }
  };
  // two pixel groups per pass: 18 loads in flight, the first group's FMAs waiting only on its own
  for (int st = 0; st < steps; st += 2) {
    u32x4 xa[9], xb[9];
    load(xa);
    const int pa = pix, ba = b, oha = oh, owa = ow;
    advance();
    if (st + 1 >= steps) pix = P;  // odd tail: the second group is empty
    load(xb);
    const int pb = pix, bb = b, ohb = oh, owb = ow;
    advance();
    finish(xa, pa, ba, oha, owa);
    finish(xb, pb, bb, ohb, owb);
  }
}

// Weight gradient of a 3x3 stride-1 pad-1 Conv2d with NC <= 4 output channels over a CW-channel
// input (CW % 4 == 0; arch 1's 3-channel output layer, GLI:222): dW[co][ci][kh][kw] = sum_p
// dy[p][co] x[p + (kh, kw) - 1][ci].  A block owns R whole output rows of one image (R * Wo <=
// N3W_PIX): it first stages their dy rows and the R + 2 x rows around them (zero halo) in LDS
// with every thread's loads in flight together, then thread (tap, 4 input channels) accumulates
// its 4 x NC outputs over the block's pixels in order from LDS.  The per-block partials go to a
// slab in the WGRAD GEMM's [split][co][(kh, kw, ci)] layout, which splitk_reduce(_wide) adds in
// block order into torch layout (and into .grad when accumulating).  As a GEMM this is M = NC:
// a 128 x 128 tile >= 97 % padding (88 us per C4 call; here 14.7 us + the reduce).  The
// mirror case (<= 4 input channels, arch 1's input layer) stays on the GEMM: the same staging
// measured 40 us per call against its 29 us (K = 9 NC is only short, M is full).
constexpr int N3W_UNR = 8;  // x-halo float4 loads in flight per thread
template <int NC>
__global__ void wgrad3_narrow(NarrowArgs a, int CW, int R) {
  extern __shared__ __attribute__((aligned(16))) float sm3[];
  const int Wo = a.Wo, XW = Wo + 2;
  float* xs = sm3;                          // [(R + 2) * XW][CW]
  float* ds = sm3 + (R + 2) * XW * CW;      // [R * Wo][NC]
  const int rows_per_img = (a.Ho + R - 1) / R, b = blockIdx.x / rows_per_img;
  const int oh0 = (blockIdx.x - b * rows_per_img) * R, nr = min(R, a.Ho - oh0);
  const int tid = threadIdx.x, nt = blockDim.x;
  // stage: x rows oh0 - 1 .. oh0 + nr (zero outside the image), dy rows oh0 .. oh0 + nr - 1
  const int xn = (R + 2) * XW * CW;
  if (a.xsc == 1 && ((a.xsw | a.xsh | a.xsb) & 3) == 0 && ((uintptr_t)a.x & 15) == 0) {
    // NHWC: float4 per (pixel, 4 channels), N3W_UNR loads in flight per thread before the LDS
    // stores (round 6: the scalar loop below kept ~1 load in flight -- 33.6 us per C4 call)
    const int CQ = CW / 4, xq = xn / 4;
    for (int i0 = tid; i0 < xq; i0 += N3W_UNR * nt) {
      float4 v[N3W_UNR];
#pragma unroll
      for (int u = 0; u < N3W_UNR; ++u) {
        const int i = i0 + u * nt;
        const int cq = i % CQ, pix = i / CQ, rr = pix / XW, cc = pix - rr * XW;
        const int ih = oh0 - 1 + rr, iw = cc - 1;
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < xq && rr < nr + 2 && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
          v[u] = *reinterpret_cast<const float4*>(a.x + (long long)b * a.xsb + (long long)ih * a.xsh +
                                                  (long long)iw * a.xsw + 4 * cq);
      }
#pragma unroll
      for (int u = 0; u < N3W_UNR; ++u)
        if (i0 + u * nt < xq) reinterpret_cast<float4*>(xs)[i0 + u * nt] = v[u];
    }
  } else {
    for (int i = tid; i < xn; i += nt) {
      const int c = i % CW, pix = i / CW, rr = pix / XW, cc = pix - rr * XW;
      const int ih = oh0 - 1 + rr, iw = cc - 1;
      xs[i] = (rr < nr + 2 && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
                  ? a.x[(long long)b * a.xsb + (long long)c * a.xsc + (long long)ih * a.xsh + (long long)iw * a.xsw]
                  : 0.f;
    }
  }
  const int dn = nr * Wo * NC;
  for (int i = tid; i < dn; i += nt) {
    const int c = i % NC, pix = i / NC, rr = pix / Wo, cc = pix - rr * Wo;
    ds[i] = a.dy[(long long)b * a.dsb + (long long)c * a.dsc + (long long)(oh0 + rr) * a.dsh + (long long)cc * a.dsw];
  }
  __syncthreads();
  const int q = tid % (CW / 4), t = tid / (CW / 4);
  if (t >= 9) return;
  const int kh = t / 3, kw = t % 3;
  float acc[4][NC];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[e][c] = 0.f;
  for (int rr = 0; rr < nr; ++rr) {
    const float* xr = xs + ((rr + kh) * XW + kw) * CW + 4 * q;
    const float* dr = ds + rr * Wo * NC;
    for (int cc = 0; cc < Wo; ++cc) {
      const float4 xv = *reinterpret_cast<const float4*>(xr + cc * CW);
      const float x4[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[e][c] += x4[e] * dr[cc * NC + c];
    }
  }
  // slab [block][co][(t, ci)]: M = NC rows of N = 9 CW
  float* sl = a.slab + (size_t)blockIdx.x * NC * 9 * CW;
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int c = 0; c < NC; ++c) sl[((size_t)c * 9 + t) * CW + 4 * q + e] = acc[e][c];
}


// Conv2d k4 s2 p1 over an image with CI <= 3 channels producing Cout % 128 == 0 channels
// NHWC (D's image layer GLI:410, and G's image-layer data gradient).  K = 16 CI is too
// short for the pipelined GEMM, and the layer both runs 6.4 GFLOP of fp32 MFMA and streams
// a 128-channel output (C3 shard: 268 MB).  Every WAVE is an independent persistent worker
// (no block barrier anywhere in the loop: the per-tile barrier of a block-shared window held
// the MFMA pipe at ~50 % through convoys of waves waiting for each other):
//   * a wave tile is 32 consecutive output pixels (a row segment, or 2 rows of 16) x the
//     block's 128 channels: 4 accumulators of 32 x 32, channels as MFMA rows;
//   * the wave's 128 x K weights (x the spectral 1/sigma) stay in VGPRs, so each MFMA step
//     reads ONE im2col operand from LDS (a ds_read_b32 at a compile-time offset) for 4
//     MFMAs; the bias is the accumulators' initial value;
//   * its input window (2R+2 rows x 2 WS+8 columns x CI, 16-B aligned) arrives by LDS-DMA
//     (buffer_load_dwordx4 ... lds into a wave-private double buffer, one tile ahead); the
//     zero padding is the buffer's out-of-range read (whole float4s lie inside or outside
//     the image: W % 4 == 0);
//   * epilogue per 32-channel group: activation, staging in a wave-private XOR-swizzled LDS
//     tile, read back as 128-B channel runs, buffer stores with SGPR offsets.
// fp32 MFMA and VALU share an issue pipe on gfx950: the VALU left is 2 per activated value
// and 4 per DMA piece; two waves per SIMD hide each other's epilogue behind their MFMAs.
// Measured at the C3 shape (32 x 3 x 256^2 -> 128 ch, tools/narrow_micro.py, HIP events
// incl. a ~6 us launch floor): 133 us for the block-tiled predecessor, 79 us here.  The
// same loop without the epilogue runs at the MFMA roof (~43 us); the prologue's weight
// staging must be bank-conflict free (row stride K + 1: an 8-way conflicted version cost
// 9 us per launch).
typedef int i32x4 __attribute__((ext_vector_type(4)));
// byte address of an LDS location, wave-uniform (M0 operand of an LDS-DMA)
__device__ __forceinline__ int lds_addr(const float* p) {
  return __builtin_amdgcn_readfirstlane((int)(uintptr_t)(const __attribute__((address_space(3))) float*)p);
}
// One 16-B-per-lane LDS-DMA piece: lane l's 16 bytes at byte offset voff of the raw buffer
// land at LDS byte m0 + 16 l (an out-of-range voff writes zeros).
__device__ __forceinline__ void dma_lds16(int m0, int voff, i32x4 rsrc) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
               :
               : "s"(m0), "v"(voff), "s"(rsrc)
               : "memory", "m0");
}

// One 16-B-per-lane buffer store (raw descriptor rsrc, per-lane voff, wave-uniform soff) followed
// by wait states IN THE SAME STATEMENT, so no instruction can sit between the store and them.
// gfx950 does not interlock a VALU write of a wide store's data VGPRs against the store still
// reading them, and LLVM inserts no wait state for a MUBUF store whose soffset is an SGPR: with
// two blocks per CU a v_mul writing the data's first VGPR right behind the store replaced the
// first dword of lanes 12-15 of every 16 (C2 / C3 image layers: 0.1-1 % of D's first-layer
// outputs wrong on every wave's second and later tiles; tools/img_in_check.py).
typedef float f32x4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store16_guarded(float4 f, int voff, i32x4 rsrc, int soff) {
  const f32x4v v = {f.x, f.y, f.z, f.w};
  asm volatile("buffer_store_dwordx4 %0, %1, %2, %3 offen\n\ts_nop 4"
               :
               : "v"(v), "v"(voff), "s"(rsrc), "s"(soff)
               : "memory");
}

// NI: 32-channel groups per block (4: 128-channel tiles; 1: 32-channel tiles for narrow D widths)
template <int CI, int WS, int ACT, int NI = 4>  // ACT 0: identity, 1: max(v, v * neg) (ReLU / LeakyReLU, neg <= 1), 2: act_fwd
__global__ __launch_bounds__(256, 2) void conv_img_in(NarrowArgs a, int tiles) {
  constexpr int NCH = 32 * NI;                    // output channels per block
  constexpr int K = CI * 16, NS = K / 2;          // MFMA steps (32x32x2)
  constexpr int RW = 32 / WS;                     // output rows per wave tile (1 or 2)
  constexpr int RR = 2 * RW + 2, CW = 2 * WS + 8; // window rows, columns (image cols 2 oj0 - 4 ..)
  constexpr int WCH = RR * CW;                    // window floats per channel
  constexpr int WIN = CI * WCH, NQ = WIN / 4;     // window floats, float4s
  constexpr int QPL = (NQ + 63) / 64;             // DMA pieces per lane
  constexpr int WSTG = (NCH * (K + 1) + 511) / 512 * 64;  // 1/8 of the prologue's weight staging
  constexpr int WBUF = QPL * 256 > WSTG ? QPL * 256 : WSTG;  // one window buffer (floats)
  constexpr int RD = 4;                           // im2col read-ahead (MFMA steps)
  constexpr int OOB_OFF = 0x7ffffff0;
  static_assert(CW % 4 == 0 && WIN % 4 == 0, "window rows are float4-aligned");
  __shared__ __attribute__((aligned(16))) float win[4][2][WBUF];
  __shared__ __attribute__((aligned(16))) float stg[4][32 * 32];  // per wave [pixel][channel quad ^ swz]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l32 = lane & 31, lk = lane >> 5;
  const int n0 = blockIdx.y * NCH;
  const int HWo = a.Ho * a.Wo;
  // raw buffer descriptor of x for the DMA pieces (stride 0, num_records = byte extent)
  const i32x4 xd = {(int)(uintptr_t)a.x, (int)((uintptr_t)a.x >> 32), a.x_bytes, 0x00020000};
  const i32x4 yd = {(int)(uintptr_t)a.y, (int)((uintptr_t)a.y >> 32), a.y_bytes, 0x00020000};
  // weights: wa[i][s] = W[n0 + 32 i + l32][2 s + lk] / sigma  (torch [Cout][CI][4][4] = [n][k])
  // (staged through LDS by the whole block with coalesced loads: NCH x K floats, once)
  // (every global load of the prologue is issued before the first wait: at ~1-2 us per
  // round trip, a dependent sequence of them costs as much as several tiles)
  constexpr int WLD = (NCH * K + 255) / 256;
  float wtmp[WLD];
#pragma unroll
  for (int q = 0; q < WLD; ++q) {
    const int e = tid + 256 * q;
    wtmp[q] = e < NCH * K ? a.w[(size_t)n0 * K + e] : 0.f;
  }
  const float wsc = a.wscale ? a.wscale[0] : 1.f;
  float wb[NI];  // bias column (see below)
#pragma unroll
  for (int i = 0; i < NI; ++i) wb[i] = (a.bias && lk == 0) ? a.bias[n0 + 32 * i + l32] : 0.f;
  {
    float* wst = &win[0][0][0];  // the window buffers are free until the first DMA
    static_assert(4 * 2 * WBUF >= NCH * (K + 1), "weight staging fits the window buffers");
#pragma unroll
    for (int q = 0; q < WLD; ++q) {
      const int e = tid + 256 * q, r = e / K;  // row stride K + 1: conflict-free reads below
      if (e < NCH * K) wst[e + r] = wtmp[q];
    }
    __syncthreads();
  }
  float wa[NI][NS];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int s = 0; s < NS; ++s) wa[i][s] = win[0][0][(32 * i + l32) * (K + 1) + 2 * s + lk];
  if (a.wscale) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int s = 0; s < NS; ++s) wa[i][s] *= wsc;
  }
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int s = 0; s < NS; ++s) asm volatile("" : "+v"(wa[i][s]));  // resident: no re-load in the loop
  // bias as one extra MFMA step per accumulator (wb: k0 = bias, k1 = 0, against a column of
  // ones): the accumulators start from it exactly, with no per-tile LDS reads
  const float one_k0 = lk == 0 ? 1.f : 0.f;
  __syncthreads();  // weight staging read before the window buffers are reused
  // this lane's pixel: row pr, column pc of the wave tile; window base of its im2col reads
  const int pr = l32 / WS, pc = l32 - pr * WS;
  const int base = 2 * pr * CW + 2 * pc + 3 + lk;
  // DMA piece q of this lane = window float4 f = 64 q + lane = (c, rr, c4): source byte offset
  // relative to the tile's (2 oi0, 2 oj0) corner, and edge flags (1 left float4, 2 right,
  // 4 top row, 8 bottom row, 16 beyond the window), 5 bits per piece
  int wofs[QPL], wflag = 0;
#pragma unroll
  for (int q = 0; q < QPL; ++q) {
    const int f = 64 * q + lane;
    const int c = f / (WCH / 4), r2 = f - c * (WCH / 4), rr = r2 / (CW / 4), c4 = r2 - rr * (CW / 4);
    wofs[q] = (int)(((long long)c * a.xsc + (long long)(rr - 1) * a.xsh + (long long)(4 * c4 - 4)) * 4);
    const int fl = f >= NQ ? 16 : (c4 == 0 ? 1 : 0) | (c4 == CW / 4 - 1 ? 2 : 0) | (rr == 0 ? 4 : 0) | (rr == RR - 1 ? 8 : 0);
    wflag |= fl << (5 * q);
  }
  auto tile_pos = [&](int t, int& b, int& oi0, int& oj0) {
    const int m0 = t * 32;
    b = m0 / HWo;
    const int rem = m0 - b * HWo;
    oi0 = rem / a.Wo;
    oj0 = rem - oi0 * a.Wo;
  };
  auto fetch = [&](int t, float* dst) {
    int b, oi0, oj0;
    tile_pos(t, b, oi0, oj0);
    const int mask = 16 | (oj0 == 0 ? 1 : 0) | (oj0 + WS >= a.Wo ? 2 : 0) | (oi0 == 0 ? 4 : 0) | (oi0 + RW >= a.Ho ? 8 : 0);
    const int tb = (int)(((long long)b * a.xsb + 2LL * oi0 * a.xsh + 2LL * oj0) * 4);
#pragma unroll
    for (int q = 0; q < QPL; ++q) {
      const int off = ((wflag >> (5 * q)) & mask) ? OOB_OFF : wofs[q] + tb;
      dma_lds16(lds_addr(dst + 256 * q), off, xd);
    }
  };
  // epilogue geometry: staging T[pixel][quad ^ ((pixel >> 1) & 7)] (conflict-free writes of
  // (pixel l32, quad 2g + lk) and reads of (pixel 8u + lane / 8, quad lane % 8)); each store
  // instruction writes 8 pixels x 128 B
  float* T = stg[wid];
  const int rq = lane & 7, rp = lane >> 3;
  const int lvo = (int)(((long long)rp * a.ysw + 4 * rq + n0) * 4);
  const int ysh4 = (int)(a.ysh * 4), ysw4 = (int)(a.ysw * 4);
  const float neg = a.act == RGAN_ACT_RELU ? 0.f : a.alpha;
  auto actf = [&](float v) {
    if constexpr (ACT == 0) return v;
    else if constexpr (ACT == 1) return vmaxf(v, v * neg);
    else return act_fwd(v, a.act, a.alpha);
  };
  const int G = (int)gridDim.x * 4;
  int t = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wid);  // wave-uniform (SGPR)
  if (t >= tiles) return;
  float* W0 = win[wid][0];
  float* W1 = win[wid][1];
  fetch(t, W0);
  // one wave tile: MFMAs from window Wr, then the next tile's window into Wn, then the
  // epilogue.  The DMA pieces are inline asm (dma_lds16), invisible to the compiler's wait
  // insertion -- which cannot tell the buffers apart and would stall every later LDS read on
  // them -- so the waits for them are the explicit vmcnt below, and nothing else in the loop
  // loads from global memory
  auto tile = [&](int t, const float* Wr, float* Wn, auto first_c) {
    const int tn = t + G;
    const bool more = tn < tiles;
    // this tile's window landed: the previous tile's 16 stores went out after its DMA and
    // may stay in flight (vmcnt retires in issue order)
    // (NI x 4 stores per tile: vmcnt(4 NI); a fixed vmcnt(16) let the 32-channel tiles read
    // their window before its DMA landed)
    constexpr int VMC = 4 * NI, VMC_ENC = 0x0f70 | (VMC & 15) | ((VMC >> 4) << 14);
    if constexpr (decltype(first_c)::value) __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0)
    else __builtin_amdgcn_s_waitcnt(VMC_ENC);                                     // vmcnt(4 NI)
    float bv[NS];
    auto read_step = [&](int s) {
      // k = 2 s + lk = 16 ci + 4 kh + kw; the lk part is in base (kw parity)
      const int k0 = 2 * s, ci = k0 >> 4, kh = (k0 >> 2) & 3, kw = k0 & 3;
      bv[s] = Wr[base + ci * WCH + kh * CW + kw];
    };
#pragma unroll
    for (int s = 0; s < RD && s < NS; ++s) read_step(s);
    f32x16 acc[NI];
    const f32x16 zero = {};
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[i], one_k0, zero, 0, 0, 0);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (s + RD < NS) read_step(s + RD);
#pragma unroll
      for (int i = 0; i < NI; ++i)
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[i][s], bv[s], acc[i], 0, 0, 0);
    }
    if (more) fetch(tn, Wn);
    int b, oi0, oj0;
    tile_pos(t, b, oi0, oj0);
    const int tb4 = (int)(((long long)b * a.ysb + (long long)oi0 * a.ysh + (long long)oj0 * a.ysw) * 4);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int quad = 2 * g + lk;
        *reinterpret_cast<float4*>(T + l32 * 32 + 4 * (quad ^ ((l32 >> 1) & 7))) =
            make_float4(actf(acc[i][4 * g]), actf(acc[i][4 * g + 1]), actf(acc[i][4 * g + 2]), actf(acc[i][4 * g + 3]));
      }
      float4 ev[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int pl = 8 * u + rp;
        ev[u] = *reinterpret_cast<const float4*>(T + pl * 32 + 4 * (rq ^ ((pl >> 1) & 7)));
      }

#pragma unroll
      for (int u = 0; u < 4; ++u) {
        // pixels 8 u .. 8 u + 7 of the wave tile lie in one output row (WS >= 16); the
        // store carries its own wait states (store16_guarded)
        const int p = 8 * u, prr = p / WS, pcc = p - prr * WS;
        const int so = __builtin_amdgcn_readfirstlane(tb4 + prr * ysh4 + pcc * ysw4 + 128 * i);
        store16_guarded(ev[u], lvo, yd, so);
      }
    }
  };
  using F = std::integral_constant<bool, false>;
  using Tr = std::integral_constant<bool, true>;
  tile(t, W0, W1, Tr{});
  for (;;) {
    t += G;
    if (t >= tiles) break;
    tile(t, W1, W0, F{});
    t += G;
    if (t >= tiles) break;
    tile(t, W0, W1, F{});
  }
}

// k4 s2 p1 ConvTranspose2d with NC <= 4 output channels on v_mfma_f32_4x4x1_16b_f32: 16
// independent 4x4 outer products per instruction, so the 4 output channels fill the N
// dimension (75% useful at NC = 3 against 9% for a 32-wide tile) and the 64 lanes are 64
// input-grid pixels: lane 4b+i supplies pixel 4b+i's input value (A row i of block b),
// lane 4b+j the weight of output channel j (B column j, the same in every block); lane
// 4b+j receives D[b][i][j] = pixel 4b+i, channel j.  Each of the 16 (phase, tap) pairs is
// one K=1 step per input channel: output (2i+ph, 2j+pw) <- input (i+ph-th, j+pw-tw) through
// tap (2th+1-ph, 2tw+1-pw), th, tw in {0, 1}.
// Block: 16 x 32 input pixels (4 waves x 2 groups of 4 x 16), the (18 x 34)-pixel halo
// staged through LDS 16 channels at a time (pixel stride 20 dwords: ds_read_b128 of 4
// channels), weights [co][c][tap] staged beside it; per 4 channels a wave reads 18 + 16
// ds_read_b128 and issues 128 MFMAs.
// (NM_TR x NM_TC input pixels per tile, NM_CH channels per staged chunk: conv_plan.h)
constexpr int NM_HR = NM_TR + 2, NM_HC = NM_TC + 2, NM_LD = NM_CH + 4;
constexpr int NM_XQ = NM_HR * NM_HC * (NM_CH / 4);  // float4 slots of one staged chunk
// LDS row stride of the staged halo: a multiple of 64 dwords, so that the two image rows a
// ds_read_b128 lane group spans (lanes 0-3 and 12-15 of one row, 20-27 of the next: the
// MI355X_MICROARCH.md LDS table) land on disjoint banks -- at the packed 680-dword stride
// (34 pixels x 20) they overlapped two ways (SQ_LDS_BANK_CONFLICT 11.9M cycles per C3 launch)
constexpr int NM_RS = (NM_HC * NM_LD + 63) / 64 * 64;
constexpr int NM_XPT = (NM_XQ + 255) / 256;         // ... per thread

typedef float f32x4 __attribute__((ext_vector_type(4)));

// 4x4x1 MFMA whose B operand is lane group g (lanes 16 g .. 16 g + 15) of b, broadcast to
// all 16 blocks (BLGP = 4 + g; g must fold to a constant)
__device__ __forceinline__ f32x4 mfma4_bcast(float a, float b, f32x4 c, int g) {
  switch (g) {
    case 0: return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 4);
    case 1: return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 5);
    case 2: return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 6);
    default: return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 7);
  }
}

template <int NC>
__global__ __launch_bounds__(256, 2) void convt2_narrow_mfma(NarrowArgs a, int ntiles) {
  __shared__ __attribute__((aligned(16))) float xs[NM_HR * NM_RS];
  __shared__ __attribute__((aligned(16))) float wl[NM_CH * 256];  // [c][r][lane] (pack_narrow order)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int tiles_c = (a.W + NM_TC - 1) / NM_TC, tiles_r = (a.H + NM_TR - 1) / NM_TR;
  const int per_img = tiles_c * tiles_r;
  const int co = lane & 3;
  // this lane's pixel in each group (tile coords): row 4 wid + lane / 16, col 16 g + lane % 16
  const int pr = 4 * wid + (lane >> 4), pc = lane & 15;
  // Persistent over (image, 16 x 32 tile) with the next channel chunk's halo and weights
  // loaded into registers while the current chunk's MFMAs run (the one-shot grid of 1024
  // blocks ran a 3-blocks-per-CU round plus a 1-block tail, every chunk's loads exposed).
  float4 stage[NM_XPT];
  float4 wv[4];
  // this thread's halo slots of the tile being prefetched: element offset of (pixel, channel
  // quad tid % 4) within the image, or -1 outside it -- computed once per tile, so a chunk's
  // prefetch is one add per load (the per-chunk index arithmetic was 1.6 VALU per MFMA, and
  // fp32 MFMA and VALU share the issue port)
  int xo[NM_XPT], sxo[NM_XPT];  // ... and its slots' LDS offsets (fixed per thread)
  const int q4 = 4 * (tid & 3);
#pragma unroll
  for (int t = 0; t < NM_XPT; ++t) {
    const int pix = (tid + 256 * t) >> 2, hr = pix / NM_HC;
    sxo[t] = hr * NM_RS + (pix - hr * NM_HC) * NM_LD + q4;
  }
  auto set_tile = [&](int r0, int c0p) {
#pragma unroll
    for (int t = 0; t < NM_XPT; ++t) {
      const int e = tid + 256 * t, pix = e >> 2;
      const int hr = pix / NM_HC, hc = pix - hr * NM_HC;
      const int ih = r0 - 1 + hr, iw = c0p - 1 + hc;
      xo[t] = (e < NM_XQ && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
                  ? ih * (int)a.xsh + iw * (int)a.xsw + q4
                  : -1;
    }
  };
  auto load_chunk = [&](const float* xb, int ch0) {
    const bool cok = ch0 + q4 < a.C;
#pragma unroll
    for (int t = 0; t < NM_XPT; ++t) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (cok && xo[t] >= 0) v = *reinterpret_cast<const float4*>(xb + xo[t] + ch0);
      stage[t] = v;
    }
    // weights: this chunk's [c][r][lane] slice of the pack, contiguous (c >= C -> 0)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = 4 * (tid + 256 * q);  // float index within the chunk's 16 x 256
      wv[q] = ch0 + (e >> 8) < a.C ? *reinterpret_cast<const float4*>(a.w + (size_t)ch0 * 256 + e)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto tile_of = [&](int t, int& b, int& r0, int& c0p) {
    b = t / per_img;
    const int trem = t - b * per_img, tr = trem / tiles_c;
    r0 = tr * NM_TR;
    c0p = (trem - tr * tiles_c) * NM_TC;
  };
  // work item = (tile, input-channel split): item = tile * splits + split.  Small grids
  // (G's 32 x 32 -> 64 x 64 image layer: 64 tiles) split the channel sum over blocks so the
  // chip is filled; the raw partial sums then go to a slab reduced in split order.
  const int items = ntiles * a.splits;
  auto item_of = [&](int it, int& t, int& cb, int& ce) {
    t = it / a.splits;
    cb = (it - t * a.splits) * a.cps;
    ce = min(a.C, cb + a.cps);
  };
  int it = blockIdx.x;
  if (it >= items) return;
  const float* xb_next;
  {
    int t, cb, ce, b, r0, c0p;
    item_of(it, t, cb, ce);
    tile_of(t, b, r0, c0p);
    set_tile(r0, c0p);
    xb_next = a.x + (long long)b * a.xsb;
    load_chunk(xb_next, cb);
  }
  for (; it < items; it += gridDim.x) {
    int t, cb, ce, b, r0, c0p;
    item_of(it, t, cb, ce);
    tile_of(t, b, r0, c0p);
    f32x4 acc[2][4];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[g][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ch0 = cb; ch0 < ce; ch0 += NM_CH) {
      const int nch = min(NM_CH, ce - ch0);
      __syncthreads();  // previous chunk's (or tile's) LDS reads are done
#pragma unroll
      for (int q = 0; q < NM_XPT; ++q) {
        const int e = tid + 256 * q;
        if (e < NM_XQ) *reinterpret_cast<float4*>(xs + sxo[q]) = stage[q];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) *reinterpret_cast<float4*>(wl + 4 * (tid + 256 * q)) = wv[q];
      __syncthreads();
      // the next chunk (or the next tile's first chunk) into registers during the MFMAs
      if (ch0 + NM_CH < ce) {
        load_chunk(xb_next, ch0 + NM_CH);
      } else if (it + (int)gridDim.x < items) {
        int t2, cb2, ce2, b2, r2, c2;
        item_of(it + (int)gridDim.x, t2, cb2, ce2);
        tile_of(t2, b2, r2, c2);
        set_tile(r2, c2);
        xb_next = a.x + (long long)b2 * a.xsb;
        load_chunk(xb_next, cb2);
      }
      for (int c4 = 0; c4 < nch / 4; ++c4) {
        float4 xv[2][3][3];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v)
              xv[g][u][v] = *reinterpret_cast<const float4*>(xs + (pr + u) * NM_RS + (16 * g + pc + v) * NM_LD + 4 * c4);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          // B operands: 4 registers of 4 taps each (one ds_read_b32 apiece: 64 distinct
          // words); the MFMA's BLGP = 4 + g broadcasts lane group g (tap 4 r + g, co = lane % 4)
          // to all 16 blocks
          float wr[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) wr[r] = wl[((4 * c4 + cc) * 4 + r) * 64 + lane];
          // (th, tw) outermost: 8 consecutive MFMAs on 8 different accumulators
#pragma unroll
          for (int th = 0; th < 2; ++th)
#pragma unroll
            for (int tw = 0; tw < 2; ++tw)
#pragma unroll
              for (int ph = 0; ph < 2; ++ph)
#pragma unroll
                for (int pw = 0; pw < 2; ++pw) {
                  const int tap = (2 * th + 1 - ph) * 4 + (2 * tw + 1 - pw);
#pragma unroll
                  for (int g = 0; g < 2; ++g) {
                    const float4 xq = xv[g][ph - th + 1][pw - tw + 1];
                    const float xa = cc == 0 ? xq.x : cc == 1 ? xq.y : cc == 2 ? xq.z : xq.w;
                    acc[g][ph * 2 + pw] = mfma4_bcast(xa, wr[tap >> 2], acc[g][ph * 2 + pw], tap & 3);
                  }
                }
        }
      }
    }
    if (co < NC && a.splits > 1) {  // raw partial sums, [split][b][co][oh][ow]
      float* sb = a.slab + ((long long)((it % a.splits) * a.B + b) * NC + co) * a.Ho * a.Wo;
      const int blk = lane >> 2;
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int q = 4 * blk + i;
          const int gi = r0 + 4 * wid + (q >> 4), gj = c0p + 16 * g + (q & 15);
          if (gi >= a.H || gj >= a.W) continue;
#pragma unroll
          for (int ph = 0; ph < 2; ++ph)
#pragma unroll
            for (int pw = 0; pw < 2; ++pw)
              sb[(long long)(2 * gi + ph) * a.Wo + 2 * gj + pw] = acc[g][ph * 2 + pw][i];
        }
    } else if (co < NC) {
      const float wsc = a.wscale ? a.wscale[0] : 1.f;
      const float bv = a.bias ? a.bias[co] : 0.f;
      float* yb = a.y + (long long)b * a.ysb + (long long)co * a.ysc;
      const int blk = lane >> 2;  // this lane holds pixels 4 blk + i of each group, channel co
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int q = 4 * blk + i;  // pixel index within the group (lane order)
          const int gi = r0 + 4 * wid + (q >> 4), gj = c0p + 16 * g + (q & 15);
          if (gi >= a.H || gj >= a.W) continue;
#pragma unroll
          for (int ph = 0; ph < 2; ++ph)
#pragma unroll
            for (int pw = 0; pw < 2; ++pw)
              yb[(long long)(2 * gi + ph) * a.ysh + (long long)(2 * gj + pw) * a.ysw] =
                  act_fwd(acc[g][ph * 2 + pw][i] * wsc + bv, a.act, a.alpha);
        }
    }
  }
}

// y = act(sum over splits of convt2_narrow_mfma's partial sums * wscale + bias), splits
// added in order (deterministic); one thread per output element, slab reads coalesced
__global__ __launch_bounds__(256) void narrow_split_reduce(NarrowArgs a) {
  const long long per = (long long)a.Ho * a.Wo, n = (long long)a.B * a.Cout * per;
  const float wsc = a.wscale ? a.wscale[0] : 1.f;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    float v = a.slab[e];
    for (int sp = 1; sp < a.splits; ++sp) v += a.slab[(long long)sp * n + e];
    const long long bc = e / per, pix = e - bc * per;
    const int b = (int)(bc / a.Cout), co = (int)(bc - (long long)b * a.Cout);
    const int oh = (int)(pix / a.Wo), ow = (int)(pix - (long long)oh * a.Wo);
    a.y[(long long)b * a.ysb + (long long)co * a.ysc + (long long)oh * a.ysh + (long long)ow * a.ysw] =
        act_fwd(v * wsc + (a.bias ? a.bias[co] : 0.f), a.act, a.alpha);
  }
}

// packed narrow-ConvT weights in MFMA B-operand lane order, [C][4][64]: register r of input
// channel ci holds, in lane l, W[ci][co = l % 4][tap = 4 r + l / 16] (co >= NC: 0, the
// MFMA's fourth column) -- lane group l / 16 is one tap, selected by the MFMA's BLGP
// broadcast (convt2_narrow_mfma)
__global__ void pack_narrow(const float* __restrict__ W, float* __restrict__ out, int C, int NC, long long s_in,
                            long long s_out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= C * 256) return;
  const int l = e & 63, r = (e >> 6) & 3, ci = e >> 8, co = l & 3, t = 4 * r + (l >> 4);
  out[e] = co < NC ? W[ci * s_in + co * s_out + t] : 0.f;
}

void launch_pack_narrow(const Plan& p, float* out, hipStream_t s) {
  const int n = p.na.C * 256;
  pack_narrow<<<ceil_div(n, 256), 256, 0, s>>>(p.pk.W, out, p.na.C, p.na.Cout, p.pn_s_in, p.pn_s_out);
}

int run_narrow(Plan& p, const float* packed, hipStream_t s) {
  NarrowArgs a = p.na;
  if (p.mode == MODE_NARROW_T) {
    a.w = packed;
    const int ntiles = a.B * ceil_div(a.H, NM_TR) * ceil_div(a.W, NM_TC);
    const int blocks = std::min(ntiles * a.splits, 512);  // persistent: two resident blocks per CU
    prof_kernel("void rgan::convt2_narrow_mfma<NC>(rgan::NarrowArgs)");
    switch (a.Cout) {
      case 1: convt2_narrow_mfma<1><<<blocks, 256, 0, s>>>(a, ntiles); break;
      case 2: convt2_narrow_mfma<2><<<blocks, 256, 0, s>>>(a, ntiles); break;
      case 3: convt2_narrow_mfma<3><<<blocks, 256, 0, s>>>(a, ntiles); break;
      default: convt2_narrow_mfma<4><<<blocks, 256, 0, s>>>(a, ntiles); break;
    }
    if (a.splits > 1) {
      const long long n = (long long)a.B * a.Cout * a.Ho * a.Wo;
      narrow_split_reduce<<<(unsigned)std::min<long long>(ceil_div(n, 256LL), 4096), 256, 0, s>>>(a);
    }
  } else if (p.img_in) {
    prof_kernel("void rgan::conv_img_in<CI, WT, ACT>(rgan::NarrowArgs)");
    // persistent waves (two resident blocks of 4 per CU) loop over the 32-pixel wave tiles
    // (32-channel tiles when the width is not a multiple of 128: D at h = 32, 64)
    const int tiles = a.B * a.Ho * a.Wo / 32;
    const bool wide = a.Cout % 128 == 0;
    const dim3 grid(std::min(ceil_div(tiles, 4), 512), a.Cout / (wide ? 128 : 32));
    const int act_kind = a.act == RGAN_ACT_NONE ? 0
                         : (a.act == RGAN_ACT_RELU || (a.act == RGAN_ACT_LRELU && a.alpha <= 1.f)) ? 1 : 2;
#define RGAN_IMG_A(CC, WW, NN)                                                            \
  switch (act_kind) {                                                                     \
    case 0: conv_img_in<CC, WW, 0, NN><<<grid, 256, 0, s>>>(a, tiles); break;             \
    case 1: conv_img_in<CC, WW, 1, NN><<<grid, 256, 0, s>>>(a, tiles); break;             \
    default: conv_img_in<CC, WW, 2, NN><<<grid, 256, 0, s>>>(a, tiles); break;            \
  }
#define RGAN_IMG(CC, NN)                                                          \
  if (a.Wo == 16) RGAN_IMG_A(CC, 16, NN) else RGAN_IMG_A(CC, 32, NN)
    if (!wide) {  // plan_narrow_in: CI == 3
      RGAN_IMG(3, 1)
    } else {
      switch (a.C) {
        case 1: RGAN_IMG(1, 4) break;
        case 2: RGAN_IMG(2, 4) break;
        default: RGAN_IMG(3, 4) break;
      }
    }
#undef RGAN_IMG
#undef RGAN_IMG_A
  } else {
    prof_kernel("void rgan::conv_narrow_in_mfma<CI>(rgan::NarrowArgs)");
    // persistent: two resident blocks per CU loop over the M tiles
    dim3 grid(std::min(ceil_div(a.B * a.Ho * a.Wo, 128), 512), ceil_div(a.Cout, 128));
    switch (a.C) {
      case 1: conv_narrow_in_mfma<1><<<grid, 256, 0, s>>>(a); break;
      case 2: conv_narrow_in_mfma<2><<<grid, 256, 0, s>>>(a); break;
      case 3: conv_narrow_in_mfma<3><<<grid, 256, 0, s>>>(a); break;
      default: conv_narrow_in_mfma<4><<<grid, 256, 0, s>>>(a); break;
    }
  }
  return 0;
}

int run_narrow3(Plan& p, hipStream_t s) {
  NarrowArgs a = p.na;
  if (p.mode == MODE_NARROW3) {
    const long long P = (long long)a.B * a.Ho * a.Wo, PW = 64 / (a.C / 4);
    const int steps = a.rows;
    const unsigned blocks = (unsigned)ceil_div(ceil_div(P, PW * steps), (long long)N3_WAVES);
    prof_kernel("void rgan::conv3_narrow_out<NC>(rgan::NarrowArgs, int)");
    switch (a.Cout) {
      case 1: conv3_narrow_out<1><<<blocks, 64 * N3_WAVES, 9 * a.C * 1 * 4, s>>>(a, steps); break;
      case 2: conv3_narrow_out<2><<<blocks, 64 * N3_WAVES, 9 * a.C * 2 * 4, s>>>(a, steps); break;
      case 3: conv3_narrow_out<3><<<blocks, 64 * N3_WAVES, 9 * a.C * 3 * 4, s>>>(a, steps); break;
      default: conv3_narrow_out<4><<<blocks, 64 * N3_WAVES, 9 * a.C * 4 * 4, s>>>(a, steps); break;
    }
    return 0;
  }
  const int threads = ceil_div(9 * (a.C / 4), 64) * 64, R = a.rows;
  const size_t lds = wgrad3_lds_bytes(R, a.Wo, a.C, a.Cout);
  prof_kernel("void rgan::wgrad3_narrow<NC>(rgan::NarrowArgs, int, int)");
  switch (a.Cout) {
    case 1: wgrad3_narrow<1><<<a.chunks, threads, lds, s>>>(a, a.C, R); break;
    case 2: wgrad3_narrow<2><<<a.chunks, threads, lds, s>>>(a, a.C, R); break;
    case 3: wgrad3_narrow<3><<<a.chunks, threads, lds, s>>>(a, a.C, R); break;
    default: wgrad3_narrow<4><<<a.chunks, threads, lds, s>>>(a, a.C, R); break;
  }
  RGAN_CHECK_LAUNCH();
  // the reduce of a WGRAD GEMM's [split][M][N] slab (plan_wgrad3_narrow set p.g up for it)
  Plan r = p;
  r.mode = MODE_WGRAD;
  r.g.slab = a.slab;
  return launch_splitk_reduce(r, s);
}

int run_dense1(const Plan& p, const float* packed, hipStream_t s) {
  DenseArgs a = p.da;
  if (p.dense_op != 2) {
    a.w = packed;
    const float* t = p.dense_op == 0 ? a.x : a.out;
    a.vec = a.xsc == 1 && a.C % 4 == 0 && a.xsb % 4 == 0 && a.xsh % 4 == 0 && a.xsw % 4 == 0 && aligned16(t);
  }
  if (p.dense_op == 0) {
    prof_kernel("void rgan::dense1_fwd<VEC>(rgan::DenseArgs)");
    if (a.vec) dense1_fwd<true><<<a.B, 1024, 0, s>>>(a);
    else dense1_fwd<false><<<a.B, 1024, 0, s>>>(a);
  } else if (p.dense_op == 1) {
    prof_kernel("void rgan::dense1_dgrad<VEC>(rgan::DenseArgs, rgan::FastDiv)");
    const uint32_t per = a.vec ? a.E / 4 : a.E, total = (uint32_t)a.B * per;
    const unsigned blocks = std::min<uint32_t>((total + 255) / 256, 8192);
    if (a.vec) dense1_dgrad<true><<<blocks, 256, 0, s>>>(a, FastDiv(per));
    else dense1_dgrad<false><<<blocks, 256, 0, s>>>(a, FastDiv(per));
  } else {
    prof_kernel("rgan::dense1_wgrad(rgan::DenseArgs)");
    dense1_wgrad<<<ceil_div(a.E, 256), 256, 0, s>>>(a);
  }
  return 0;
}

}  // namespace rgan
