// The passes that finish a GEMM's output: the split-K reduces (plain, wide, with BatchNorm sums)
// and the tap transpose of a staged weight gradient, with their launchers.
#include "conv_plan.h"
#include "gemm_body.h"  // row_offset, col_offset, post_seg, post_consts

namespace rgan {

// Split-K reduce: out = act(sum_sp slab[sp] * wscale + bias), slabs summed in split order
// (deterministic; loads issued 4 splits ahead of the adds).  Three shapes, chosen on the
// host:
//  RED_VEC  channel-contiguous outputs (tc == 1, 16-B aligned): one thread per (phase, m,
//           4 consecutive n), float4 loads and stores;
//  RED_TAPS torch weight layout (WGRAD, n = (kh, kw, c) over a 4x4 kernel, out[m][c][kh][kw]):
//           one thread per (m, c, 4 taps), 4 taps of a channel = one float4 store (lanes on
//           consecutive tap quads write contiguously);
//  RED_ANY  anything else, one element per thread.
enum { RED_ANY = 0, RED_VEC = 1, RED_TAPS = 2 };

__device__ __forceinline__ float red_epi(const GemmArgs& g, float v, float wsc, int n) {
  v *= wsc;
  if (g.bias) v += g.bias[n];
  return act_fwd(v, g.act, g.alpha);
}

// sum over splits of V-wide vectors at s + sp * stride, in split order
template <int V>
__device__ __forceinline__ void red_sum(const float* s, size_t stride, int splits, float (&v)[V]) {
  float t[4][V];
#pragma unroll
  for (int i = 0; i < V; ++i) v[i] = 0.f;
  int sp = 0;
  for (; sp + 4 <= splits; sp += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(s + (size_t)(sp + u) * stride);
        t[u][0] = q.x; t[u][1] = q.y; t[u][2] = q.z; t[u][3] = q.w;
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i) t[u][i] = s[(size_t)(sp + u) * stride + i];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < V; ++i) v[i] = sp + u == 0 ? t[u][i] : v[i] + t[u][i];
  }
  for (; sp < splits; ++sp)
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = sp == 0 ? s[(size_t)sp * stride + i] : v[i] + s[(size_t)sp * stride + i];
}

// split FAST conv WGRAD with a bias: dbias[m] (+)= sum over splits of dbp[split][m] in split
// order (double), by the first block of the WGRAD reduce
__device__ __forceinline__ void wgrad_db_finish(const GemmArgs& g) {
  if (g.dbias == nullptr || blockIdx.x != 0 || blockIdx.y != 0) return;
  for (int m = threadIdx.x; m < g.M; m += blockDim.x) {
    double v = 0.0;
    for (int sp = 0; sp < g.splits; ++sp) v += g.dbp[(size_t)sp * g.M + m];
    g.dbias[m] = g.db_accum ? g.dbias[m] + (float)v : (float)v;
  }
}

template <int MODE, int KIND>
__global__ __launch_bounds__(256) void splitk_reduce(GemmArgs g, FastDiv fdiv, uint32_t per_phase) {
  if constexpr (MODE == MODE_WGRAD) wgrad_db_finish(g);
  const int phase = blockIdx.y;
  const size_t MN = (size_t)g.M * g.N;
  const float* base = g.slab + (size_t)phase * g.splits * MN;
  // the unsplit epilogue computes acc * wsc + bias; wsc = 1 multiplies exactly
  const float wsc = g.wscale ? g.wscale[0] : 1.f;
  for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < per_phase; idx += gridDim.x * 256u) {
    if constexpr (KIND == RED_VEC) {
      const uint32_t m = fdiv.div(idx);               // fdiv = N / 4
      const int n = 4 * (int)(idx - m * fdiv.d);
      float v[4];
      red_sum<4>(base + (size_t)m * g.N + n, MN, g.splits, v);
      float4 o = make_float4(red_epi(g, v[0], wsc, n), red_epi(g, v[1], wsc, n + 1),
                             red_epi(g, v[2], wsc, n + 2), red_epi(g, v[3], wsc, n + 3));
      const long long ooff = row_offset(g.out, (int)m, MODE == MODE_CONVT2 ? phase : 0) + col_offset(g.out, n);
      float4* dst = reinterpret_cast<float4*>(g.C + ooff);
      if (MODE != MODE_WGRAD && g.pmode == 1) {
        const float4 a = *reinterpret_cast<const float4*>(g.px + ooff);
        o.x *= act_grad_from_out(a.x, g.pact, g.palpha);
        o.y *= act_grad_from_out(a.y, g.pact, g.palpha);
        o.z *= act_grad_from_out(a.z, g.pact, g.palpha);
        o.w *= act_grad_from_out(a.w, g.pact, g.palpha);
      }
      if (g.accum) {
        const float4 q = *dst;
        *dst = make_float4(q.x + o.x, q.y + o.y, q.z + o.z, q.w + o.w);
      } else {
        *dst = o;
      }
    } else if constexpr (KIND == RED_TAPS) {
      const uint32_t mc = idx >> 2;                   // fdiv = channels c
      const int q = (int)(idx & 3);                   // taps 4q .. 4q+3 (kh = q)
      const uint32_t m = fdiv.div(mc);
      const int c = (int)(mc - m * fdiv.d);
      const float* s = base + (size_t)m * g.N + c;
      const int nc = (int)fdiv.d;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float w[1];
        red_sum<1>(s + (size_t)(4 * q + i) * nc, MN, g.splits, w);
        v[i] = red_epi(g, w[0], wsc, (4 * q + i) * nc + c);
      }
      float4* dst = reinterpret_cast<float4*>(g.C + (long long)m * g.out.sb + (long long)c * 16 + 4 * q);
      if (g.accum) {
        const float4 o = *dst;
        v[0] += o.x; v[1] += o.y; v[2] += o.z; v[3] += o.w;
      }
      *dst = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      const uint32_t m = fdiv.div(idx);               // fdiv = N
      const int n = (int)(idx - m * fdiv.d);
      float v[1];
      red_sum<1>(base + (size_t)m * g.N + n, MN, g.splits, v);
      const long long ooff = row_offset(g.out, (int)m, MODE == MODE_CONVT2 ? phase : 0) + col_offset(g.out, n);
      float* dst = g.C + ooff;
      float o = red_epi(g, v[0], wsc, n);
      if (MODE != MODE_WGRAD && g.pmode == 1) o *= act_grad_from_out(g.px[ooff], g.pact, g.palpha);
      *dst = g.accum ? *dst + o : o;
    }
  }
}

// RED_ANY shape with few outputs and many splits (the 1x1 patch GEMMs' weight gradients: a
// 128 x 64 output, split-K 512 ways): one thread per output would be a 512-long chain on
// 32 blocks.  Here a block = 16 outputs x 16 split lanes; lane l sums splits l, l + 16, ...
// in order (4 loads in flight), then a fixed LDS tree adds the 16 lane sums (deterministic;
// a different association than red_sum's split order, the same set of fp32 partials).
constexpr int REDW_OUT = 16, REDW_LANES = 16;
template <int MODE>
__global__ __launch_bounds__(256) void splitk_reduce_wide(GemmArgs g, FastDiv fdiv, uint32_t per_phase) {
  if constexpr (MODE == MODE_WGRAD) wgrad_db_finish(g);
  __shared__ float sh[REDW_LANES][REDW_OUT + 1];
  const int phase = blockIdx.y, ob = threadIdx.x % REDW_OUT, l = threadIdx.x / REDW_OUT;
  const size_t MN = (size_t)g.M * g.N;
  const uint32_t idx = blockIdx.x * REDW_OUT + ob;
  const bool live = idx < per_phase;
  const float* s = g.slab + (size_t)phase * g.splits * MN + (live ? idx : 0);  // idx = m N + n
  float acc = 0.f;
  if (live) {
    int sp = l;
    for (; sp + 3 * REDW_LANES < g.splits; sp += 4 * REDW_LANES) {
      float t[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) t[u] = s[(size_t)(sp + u * REDW_LANES) * MN];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += t[u];
    }
    for (; sp < g.splits; sp += REDW_LANES) acc += s[(size_t)sp * MN];
  }
  sh[l][ob] = acc;
  __syncthreads();
  for (int h = REDW_LANES / 2; h > 0; h >>= 1) {
    if (l < h) sh[l][ob] += sh[l + h][ob];
    __syncthreads();
  }
  if (l == 0 && live) {
    const uint32_t m = fdiv.div(idx);  // fdiv = N
    const int n = (int)(idx - m * fdiv.d);
    const float wsc = g.wscale ? g.wscale[0] : 1.f;
    const long long ooff = row_offset(g.out, (int)m, MODE == MODE_CONVT2 ? phase : 0) + col_offset(g.out, n);
    float* dst = g.C + ooff;
    float o = red_epi(g, sh[0][ob], wsc, n);
    if (MODE != MODE_WGRAD && g.pmode == 1) o *= act_grad_from_out(g.px[ooff], g.pact, g.palpha);
    *dst = g.accum ? *dst + o : o;
  }
}

// Split-K reduce of a BatchNorm layer's conv forward with the batch statistics fused in:
// the same rows the RED_VEC reduce writes (same split order, bitwise the same values), plus
// the (sum y, sum y^2) of every 64-row segment of every channel in double -- the layout the
// unsplit vector epilogue writes (bnp[(seg * 2 + {0,1}) * N + n], seg = phase * (M / 64) +
// m / 64), so one segment merge serves both and the separate moments pass over y (4 B/elem
// + a launch) is gone.  Block = one 64-row segment x 4*qb columns, thread (rl, q) reduces
// rows rl and rl + RL (RL = 256 / qb) of quad q -- both rows' split loads in flight together,
// as many threads as the plain reduce -- then the per-thread double sums are added over rl
// by a fixed LDS tree (deterministic).  grid = (segments * column chunks, phases); qb <= REDBN_QB
// (conv_plan.h).
//
// BWD (pmode 2, the producer's BatchNorm backward sums -- see GemmArgs::pmode): the rows
// written are g = v * act'(y al + be) and the segment sums are (sum g, sum g (y - mean)),
// y read at the rows' own offsets; the same block / tree structure.
template <bool BWD>
__global__ __launch_bounds__(256) void splitk_reduce_bn(GemmArgs g, int mode_t2, int qb) {
  __shared__ double sh[2][256][4];
  const int phase = blockIdx.y;
  const int Q = g.N >> 2, chunks = (Q + qb - 1) / qb;
  const int segm = blockIdx.x / chunks, chunk = blockIdx.x - segm * chunks;
  const int tid = threadIdx.x, lq = tid % qb, q = chunk * qb + lq, rl = tid / qb, RL = 256 / qb;
  const size_t MN = (size_t)g.M * g.N;
  const float* base = g.slab + (size_t)phase * g.splits * MN;
  const float wsc = g.wscale ? g.wscale[0] : 1.f;
  double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  if (q < Q) {
    const int n = 4 * q;
    const long long noff = col_offset(g.out, n);
    float p_al[4], p_be[4], p_mu[4];
    if constexpr (BWD) {
      const int k = post_seg(g, segm * 64);
#pragma unroll
      for (int i = 0; i < 4; ++i) post_consts(g, k, n + i, p_al[i], p_be[i], p_mu[i]);
    }
    for (int r0 = rl; r0 < 64; r0 += 2 * RL) {  // RL <= 32: two rows per pass
      const int m0 = segm * 64 + r0, m1 = m0 + RL;
      const float* p0 = base + (size_t)m0 * g.N + n;
      const float* p1 = base + (size_t)m1 * g.N + n;
      float4 v0 = *reinterpret_cast<const float4*>(p0), v1 = *reinterpret_cast<const float4*>(p1);
      int sp = 1;
      for (; sp + 4 <= g.splits; sp += 4) {  // split order, as red_sum: 8 loads in flight, then the adds
        float4 a0[4], a1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          a0[u] = *reinterpret_cast<const float4*>(p0 + (size_t)(sp + u) * MN);
          a1[u] = *reinterpret_cast<const float4*>(p1 + (size_t)(sp + u) * MN);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          v0.x += a0[u].x; v0.y += a0[u].y; v0.z += a0[u].z; v0.w += a0[u].w;
          v1.x += a1[u].x; v1.y += a1[u].y; v1.z += a1[u].z; v1.w += a1[u].w;
        }
      }
      for (; sp < g.splits; ++sp) {
        const float4 a0 = *reinterpret_cast<const float4*>(p0 + (size_t)sp * MN);
        const float4 a1 = *reinterpret_cast<const float4*>(p1 + (size_t)sp * MN);
        v0.x += a0.x; v0.y += a0.y; v0.z += a0.z; v0.w += a0.w;
        v1.x += a1.x; v1.y += a1.y; v1.z += a1.z; v1.w += a1.w;
      }
      const float4 o0 = make_float4(red_epi(g, v0.x, wsc, n), red_epi(g, v0.y, wsc, n + 1),
                                    red_epi(g, v0.z, wsc, n + 2), red_epi(g, v0.w, wsc, n + 3));
      const float4 o1 = make_float4(red_epi(g, v1.x, wsc, n), red_epi(g, v1.y, wsc, n + 1),
                                    red_epi(g, v1.z, wsc, n + 2), red_epi(g, v1.w, wsc, n + 3));
      const long long off0 = row_offset(g.out, m0, mode_t2 ? phase : 0) + noff;
      const long long off1 = row_offset(g.out, m1, mode_t2 ? phase : 0) + noff;
      float a[2][4] = {{o0.x, o0.y, o0.z, o0.w}, {o1.x, o1.y, o1.z, o1.w}};
      if constexpr (BWD) {
        const float4 y0 = *reinterpret_cast<const float4*>(g.px + off0);
        const float4 y1 = *reinterpret_cast<const float4*>(g.px + off1);
        const float yy[2][4] = {{y0.x, y0.y, y0.z, y0.w}, {y1.x, y1.y, y1.z, y1.w}};
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            a[h][i] *= act_grad_from_in(yy[h][i] * p_al[i] + p_be[i], g.pact, g.palpha);
            s1[i] += (double)a[h][i];
            s2[i] += (double)a[h][i] * (double)(yy[h][i] - p_mu[i]);
          }
      } else {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const double d = (double)a[h][i];
            s1[i] += d;
            s2[i] += d * d;
          }
      }
      *reinterpret_cast<float4*>(g.C + off0) = make_float4(a[0][0], a[0][1], a[0][2], a[0][3]);
      *reinterpret_cast<float4*>(g.C + off1) = make_float4(a[1][0], a[1][1], a[1][2], a[1][3]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) { sh[0][tid][i] = s1[i]; sh[1][tid][i] = s2[i]; }
  __syncthreads();
  for (int h = RL / 2; h > 0; h >>= 1) {  // tid = rl * qb + lq: partner rl + h
    if (rl < h) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sh[0][tid][i] += sh[0][tid + h * qb][i];
        sh[1][tid][i] += sh[1][tid + h * qb][i];
      }
    }
    __syncthreads();
  }
  if (rl == 0 && q < Q) {
    const size_t seg = (size_t)phase * (uint32_t)(g.M >> 6) + (uint32_t)segm;
    double* out = BWD ? g.ppart : g.bnp;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      out[(seg * 2) * g.N + 4 * q + i] = sh[0][tid][i];
      out[(seg * 2 + 1) * g.N + 4 * q + i] = sh[1][tid][i];
    }
  }
}

// WGRAD with 4x4 taps: the GEMM writes C[co][(tap, ci)] with whole-row float4 stores
// (tap-major staging) and this pass turns it into torch layout dW[co][ci][tap].  Writing
// torch layout from the GEMM directly scatters 4-B stores at a 64-B stride (a tile covers
// one tap); on the deep layers (N = 16 Cin up to 16384) that cost ~20 % of the GEMM.
// 16 taps x 64 channels per block through LDS; reads 256-B rows, writes 4 KiB runs.
constexpr int TT_LD = 68;  // (16 t + ci) distinct mod 64 on the read side
__global__ __launch_bounds__(256) void taps_transpose(const float* __restrict__ T, float* __restrict__ O, int Cin,
                                                      long long osb, int accum) {
  __shared__ float sh[16 * TT_LD];
  const int co = blockIdx.y, c0 = blockIdx.x * 64;
  const float* src = T + (size_t)co * 16 * Cin;
  {
    const int t = threadIdx.x >> 4, q = threadIdx.x & 15, c = c0 + 4 * q;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < Cin) v = *reinterpret_cast<const float4*>(src + (size_t)t * Cin + c);
    sh[t * TT_LD + 4 * q] = v.x; sh[t * TT_LD + 4 * q + 1] = v.y;
    sh[t * TT_LD + 4 * q + 2] = v.z; sh[t * TT_LD + 4 * q + 3] = v.w;
  }
  __syncthreads();
  const int ci = threadIdx.x >> 2, tq = threadIdx.x & 3;
  if (c0 + ci < Cin) {
    float4* dst = reinterpret_cast<float4*>(O + (long long)co * osb + (long long)(c0 + ci) * 16 + 4 * tq);
    float4 v = make_float4(sh[(4 * tq) * TT_LD + ci], sh[(4 * tq + 1) * TT_LD + ci], sh[(4 * tq + 2) * TT_LD + ci],
                           sh[(4 * tq + 3) * TT_LD + ci]);
    if (accum) {
      const float4 o = *dst;
      v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
    }
    *dst = v;
  }
}

// a staged [M][16 Cin] weight gradient T into torch layout at O (row stride osb)
void launch_taps_transpose(const float* T, float* O, int M, int Cin, long long osb, int accum, hipStream_t s) {
  taps_transpose<<<dim3(ceil_div(Cin, 64), M), 256, 0, s>>>(T, O, Cin, osb, accum);
}

// The reduce of a split plan's slabs (p.mode one of the three GEMM modes; wgrad3_narrow's slabs
// come as MODE_WGRAD, see run_narrow3).
int launch_splitk_reduce(const Plan& p, hipStream_t s) {
  const GemmArgs& g = p.g;
  int kind = RED_ANY;
  uint32_t per = (uint32_t)g.M * g.N, d = g.N;
  if (vec_out(p, true)) {
    kind = RED_VEC;
    per /= 4;
    d = g.N / 4;
  } else if (p.mode == MODE_WGRAD && taps4x4_out(g) && aligned16(g.C)) {  // float4 stores: the pointer too
    kind = RED_TAPS;
    per /= 4;
    d = g.out.fnc.d;
  }
  if (p.bn_fused || g.pmode == 2) {  // the RED_VEC shape with segment moments / backward sums
    const int Q = g.N / 4;
    int qb = 1;  // quads per block: 8 (32 channels, 128-B row pieces), fewer for narrow N
    while (qb * 2 <= std::min(Q, REDBN_QB)) qb *= 2;
    const dim3 bgrid((unsigned)((g.M / 64) * ceil_div(Q, qb)), p.phases);
    if (g.pmode == 2) splitk_reduce_bn<true><<<bgrid, 256, 0, s>>>(g, p.mode == MODE_CONVT2, qb);
    else splitk_reduce_bn<false><<<bgrid, 256, 0, s>>>(g, p.mode == MODE_CONVT2, qb);
    RGAN_CHECK_LAUNCH();
    return 0;
  }
  const FastDiv fd(d);
  if (kind == RED_ANY && g.splits >= 4 * REDW_LANES && per <= 65536) {  // few outputs, long chains
    const dim3 wgrid((unsigned)ceil_div((long long)per, REDW_OUT), p.phases);
    switch (p.mode) {
      case MODE_CONV: splitk_reduce_wide<MODE_CONV><<<wgrid, 256, 0, s>>>(g, fd, per); break;
      case MODE_CONVT2: splitk_reduce_wide<MODE_CONVT2><<<wgrid, 256, 0, s>>>(g, fd, per); break;
      default: splitk_reduce_wide<MODE_WGRAD><<<wgrid, 256, 0, s>>>(g, fd, per); break;
    }
    RGAN_CHECK_LAUNCH();
    return 0;
  }
  const dim3 rgrid((unsigned)std::min<uint32_t>((per + 255) / 256, 8192), p.phases);
#define RGAN_RED(MD)                                                                   \
  switch (kind) {                                                                      \
    case RED_VEC: splitk_reduce<MD, RED_VEC><<<rgrid, 256, 0, s>>>(g, fd, per); break;  \
    case RED_TAPS: splitk_reduce<MD, RED_TAPS><<<rgrid, 256, 0, s>>>(g, fd, per); break; \
    default: splitk_reduce<MD, RED_ANY><<<rgrid, 256, 0, s>>>(g, fd, per); break;       \
  }
  switch (p.mode) {
    case MODE_CONV: RGAN_RED(MODE_CONV) break;
    case MODE_CONVT2: RGAN_RED(MODE_CONVT2) break;
    default: RGAN_RED(MODE_WGRAD) break;
  }
#undef RGAN_RED
  RGAN_CHECK_LAUNCH();
  return 0;
}

}  // namespace rgan
