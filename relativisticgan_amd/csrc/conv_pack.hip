// Weight packing: the kernels that write the GEMM-ready weight layouts (PackArgs: conv_plan.h), the
// Adam step that writes them in passing, their launchers and the pack entry points.
#include "conv_plan.h"

#include <vector>

namespace rgan {

// out[phase][n][k] (k contiguous: the GEMM B operand's rows): threads over k, one block
// column per n (n-decomposition uniform per block)
__global__ __launch_bounds__(256) void pack_weights(PackArgs a) {
  const int phase = blockIdx.z;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= a.K) return;
  for (int n = blockIdx.y; n < a.N; n += gridDim.y) {
    uint32_t tn = a.fnco.div(n);
    const int co = n - tn * a.fnco.d;
    uint32_t nh = a.fnkw.div(tn);
    const int nw = tn - nh * a.fnkw.d;
    uint32_t t = a.fpci.div(k);
    const int ci = k - t * a.fpci.d;
    int kh, kw, c_out;
    if (a.convt2) {
      kh = 2 * (int)(t >> 1) + 1 - (phase >> 1);
      kw = 2 * (int)(t & 1) + 1 - (phase & 1);
      c_out = n;
    } else {
      uint32_t kkh = a.fpkw.div(t);
      kh = (int)kkh + (int)nh;
      kw = (int)(t - kkh * a.fpkw.d) + nw;
      c_out = co;
      if (a.flip) {
        kh = a.KH - 1 - kh;
        kw = a.KW - 1 - kw;
      }
    }
    a.out[((size_t)phase * a.N + n) * a.K + k] =
        a.W[ci * a.s_in + c_out * a.s_out + kh * a.s_kh + kw * a.s_kw];
  }
}

// G's 1x1 -> KH x KW first layer (a plain GEMM over z): W[ci][co][tap] contiguous ->
// out[tap * Cout + co][ci] -- a 2-D transpose of [K][N] with the (co, tap) -> (tap, co)
// column permutation.  pack_weights reads that layout a float per 128-B line (one column
// of a K x N matrix per block); here a block moves a 32 (ci) x 128 (co, tap) brick through
// LDS, loaded as float4 rows, stored as 128-B ci runs.
__global__ __launch_bounds__(256) void pack_t2d(PackArgs a) {
  __shared__ float t[PT_K][PT_N + 1];
  const int T = a.KH * a.KW, Cout = (int)a.fnco.d;
  const int k0 = blockIdx.y * PT_K, j0 = blockIdx.x * PT_N;
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (tid >> 5) + 8 * i, c = 4 * (tid & 31);
    const float4 v = *reinterpret_cast<const float4*>(a.W + (size_t)(k0 + r) * a.N + j0 + c);
    t[r][c] = v.x; t[r][c + 1] = v.y; t[r][c + 2] = v.z; t[r][c + 3] = v.w;
  }
  __syncthreads();
  const int jl = tid >> 1, h = tid & 1, j = j0 + jl;
  const int co = j / T, tap = j - co * T;
  float* dst = a.out + (size_t)(tap * Cout + co) * a.K + k0 + 16 * h;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    *reinterpret_cast<float4*>(dst + 4 * q) = make_float4(t[16 * h + 4 * q][jl], t[16 * h + 4 * q + 1][jl],
                                                          t[16 * h + 4 * q + 2][jl], t[16 * h + 4 * q + 3][jl]);
}

// Tiled pack for the layouts whose columns are one weight index (n = out_idx) and whose
// rows are (tap, in_idx) with in_idx fastest -- every pack on the FAST paths: a block
// moves a 32 in x 8 out x (<= 16 taps) brick through LDS, reading W in its own contiguous
// order (taps, then the smaller-stride index: 512 or 128 contiguous floats) and writing
// whole 128-B lines (32-float k runs) of the [N][K] image.
constexpr int PK_LD = PK_O * 17 + 1;  // odd row stride: conflict-free reads
__device__ __forceinline__ void pack_tiled_body(const PackArgs& a, int bx, int by, float* t) {  // t: [in][out][tap]
  const int KK = a.KH * a.KW;
  const int Nin = (int)a.fpci.d, Nout = a.N;
  const int i0 = bx * PK_I, o0 = by * PK_O;
  const bool in_fast = a.s_in < a.s_out;
  for (int e = threadIdx.x; e < PK_I * PK_O * 16; e += 256) {
    const int tap = e & 15;
    const int i = in_fast ? (e >> 4) & (PK_I - 1) : e >> 7;
    const int o = in_fast ? e >> 9 : (e >> 4) & (PK_O - 1);
    float val = 0.f;
    if (tap < KK && i0 + i < Nin && o0 + o < Nout)
      val = a.W[(long long)(i0 + i) * a.s_in + (long long)(o0 + o) * a.s_out + tap];
    t[i * PK_LD + o * 17 + tap] = val;
  }
  __syncthreads();
  const int K = a.K;
  for (int e = threadIdx.x; e < PK_I * PK_O * 16; e += 256) {
    const int i = e & (PK_I - 1), o = (e >> 5) & (PK_O - 1), tap = e >> 8;
    if (tap >= KK || i0 + i >= Nin || o0 + o >= Nout) continue;
    const int kh = tap / a.KW, kw = tap - (tap / a.KW) * a.KW;
    int phase = 0, kt;
    if (a.convt2) {  // tap (kh, kw) of phase (ph, pw) = (2th+1-ph, 2tw+1-pw)
      phase = (1 - (kh & 1)) * 2 + (1 - (kw & 1));
      kt = (kh >> 1) * 2 + (kw >> 1);
    } else {
      kt = a.flip ? (a.KH - 1 - kh) * a.KW + (a.KW - 1 - kw) : tap;
    }
    a.out[((size_t)phase * Nout + o0 + o) * K + (size_t)kt * Nin + i0 + i] = t[i * PK_LD + o * 17 + tap];
  }
}

__global__ __launch_bounds__(256) void pack_tiled(PackArgs a) {
  __shared__ float t[PK_I * PK_LD];
  pack_tiled_body(a, blockIdx.x, blockIdx.y, t);
}

// 4x4 taps, Nin % 32 == 0, Nout % 8 == 0 (every C2 pack): the same brick moved with
// float4s -- 4 taps per load (taps are the weight's contiguous index), 4 in-indices per
// store (the packed row's contiguous index) -- 4 loads + 4 stores per thread, all issued
// before their first use.
constexpr int P4_LD = PK_O * 16 + 4;  // [in][out][16 taps], 16-B aligned rows
__device__ __forceinline__ void pack_tiled16_body(const PackArgs& a, int bx, int by, float* t) {
  const int Nin = (int)a.fpci.d, Nout = a.N, K = a.K;
  const int i0 = bx * PK_I, o0 = by * PK_O;
  const bool in_fast = a.s_in < a.s_out;
  float4 v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = threadIdx.x + 256 * r;  // float4 index in the brick
    const int tq = e & 3;
    const int i = in_fast ? (e >> 2) & (PK_I - 1) : e >> 5;
    const int o = in_fast ? e >> 7 : (e >> 2) & (PK_O - 1);
    v[r] = *reinterpret_cast<const float4*>(a.W + (long long)(i0 + i) * a.s_in + (long long)(o0 + o) * a.s_out +
                                            4 * tq);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = threadIdx.x + 256 * r;
    const int tq = e & 3;
    const int i = in_fast ? (e >> 2) & (PK_I - 1) : e >> 5;
    const int o = in_fast ? e >> 7 : (e >> 2) & (PK_O - 1);
    *reinterpret_cast<float4*>(t + i * P4_LD + o * 16 + 4 * tq) = v[r];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = threadIdx.x + 256 * r;
    const int iq = e & 7, o = (e >> 3) & (PK_O - 1), tap = e >> 6;
    const int kh = tap >> 2, kw = tap & 3;
    int phase = 0, kt;
    if (a.convt2) {  // tap (kh, kw) of phase (ph, pw) = (2th+1-ph, 2tw+1-pw)
      phase = (1 - (kh & 1)) * 2 + (1 - (kw & 1));
      kt = (kh >> 1) * 2 + (kw >> 1);
    } else {
      kt = a.flip ? 15 - tap : tap;
    }
    const float* src = t + (4 * iq) * P4_LD + o * 16 + tap;
    *reinterpret_cast<float4*>(a.out + ((size_t)phase * Nout + o0 + o) * K + (size_t)kt * Nin + i0 + 4 * iq) =
        make_float4(src[0], src[P4_LD], src[2 * P4_LD], src[3 * P4_LD]);
  }
}

__global__ __launch_bounds__(256) void pack_tiled16(PackArgs a) {
  __shared__ __attribute__((aligned(16))) float t[PK_I * P4_LD];
  pack_tiled16_body(a, blockIdx.x, blockIdx.y, t);
}

// Every stale weight layout of a net after its optimizer step in one launch (the repacks
// of a small model are ~10 us launches of ~1 us of work each): entry j owns blocks
// [first[j], first[j+1]) of a 1-D grid, its own (bx, by) brick grid and kernel body.
constexpr int PACK_BATCH = 16;
struct PackBatch {
  PackArgs a[PACK_BATCH];
  int kind[PACK_BATCH];  // 0: pack_tiled16, 1: pack_tiled
  int gx[PACK_BATCH];
  int first[PACK_BATCH + 1];
  int n;
};

__global__ __launch_bounds__(256) void pack_multi(PackBatch b) {
  __shared__ __attribute__((aligned(16))) float t[PK_I * (P4_LD > PK_LD ? P4_LD : PK_LD)];
  int j = 0;
  while (j + 1 < b.n && (int)blockIdx.x >= b.first[j + 1]) ++j;
  const int local = (int)blockIdx.x - b.first[j], bx = local % b.gx[j], by = local / b.gx[j];
  if (b.kind[j] == 0) pack_tiled16_body(b.a[j], bx, by, t);
  else pack_tiled_body(b.a[j], bx, by, t);
}

// ---------------------------------------------------------------- Adam writing the GEMM layouts
// The optimizer step (GLI:659, 712) rewrites every weight; the conv GEMMs read packed copies
// ([phase][N][K], tiled16 / t2d / narrow layouts above).  Re-reading each weight after Adam
// to repack it cost 8 B per weight element and a launch per net (pack_multi: 2.9 GB, 0.57 ms
// per C3 iteration); here the Adam kernel writes the packed copies of the values it has in
// registers.  Weight viewed [A][B][KK] (contiguous); per cached layout:
//   APK_TILED   out[((phase Nout + o) K + kt Nin + i)], (i, o) = (a, b) or (b, a), the tap
//               -> (phase, kt) map of pack_tiled_body (flip / 4 sub-pixel phases);
//   APK_T2D     out[(tap Cout + co) K + ci]  (G's 1x1 -> 4x4 first layer, pack_t2d);
//   APK_NARROW  out[ci 256 + (t >> 2) 64 + (t & 3) 16 + x 4 + co], x = 0..3 (pack_narrow).
// A tensor whose layouts are all 4x4-tap tiled with A, B multiples of 32 runs as 32 x 32 x 16
// bricks: Adam on the brick (coalesced 2-KB rows), the new values into LDS, then each layout
// written as float4 runs of 4 consecutive in-indices (pack_tiled16's store pattern); other
// tensors run the flat 4096-element blocks of adam_kernel with per-element scatters.
enum { APK_TILED = 0, APK_T2D = 1, APK_NARROW = 2 };
struct AdamPackT {
  float* out;
  int kind, in_is_a, A, B, KK, KW, flip, convt2, Nin, Nout, K, NC;
};
struct AdamPackTensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  long long n;
  int brick, bricks_b, pk0, npk;
};
// 1024 threads: a brick's 4096 float4 (or a flat block's 16384 elements) are one pass of 4
// float4 loads per thread and array, all in flight together (two 68-KB blocks per CU)
constexpr int AP_MAXT = 24, AP_MAXP = 24, AP_BRICK = 32 * 32 * 16, AP_FLAT = 16384, AP_TLD = 32 * 17 + 4,
              AP_THREADS = 1024;
struct AdamPackBatch {
  AdamPackTensor t[AP_MAXT];
  AdamPackT pk[AP_MAXP];
  int first[AP_MAXT + 1];
  int cnt;
};

__device__ __forceinline__ long long apk_tiled_dst(const AdamPackT& t, int a, int b, int tap) {
  const int i = t.in_is_a ? a : b, o = t.in_is_a ? b : a;
  const int kh = tap / t.KW, kw = tap - kh * t.KW;
  int phase = 0, kt;
  if (t.convt2) {
    phase = (1 - (kh & 1)) * 2 + (1 - (kw & 1));
    kt = (kh >> 1) * 2 + (kw >> 1);
  } else {
    kt = t.flip ? t.KK - 1 - tap : tap;
  }
  return ((long long)phase * t.Nout + o) * t.K + (long long)kt * t.Nin + i;
}

// brick path: destination of element (a, b, tap) of a TILED or T2D layout
__device__ __forceinline__ long long apk_brick_dst(const AdamPackT& t, int a, int b, int tap) {
  if (t.kind == APK_T2D) return ((long long)tap * t.B + b) * t.K + a;
  return apk_tiled_dst(t, a, b, tap);
}

// element e (flat index of the [A][B][KK] weight) with its new value into one layout
__device__ __forceinline__ void apk_scatter(const AdamPackT& t, long long e, float val) {
  const int tap = (int)(e % t.KK);
  const long long r = e / t.KK;
  const int a = (int)(r / t.B), b = (int)(r - (long long)a * t.B);
  if (t.kind == APK_TILED) {
    t.out[apk_tiled_dst(t, a, b, tap)] = val;
  } else if (t.kind == APK_T2D) {
    t.out[((long long)tap * t.B + b) * t.K + a] = val;
  } else {
    const long long o = (long long)a * 256 + (tap >> 2) * 64 + (tap & 3) * 16 + b;
#pragma unroll
    for (int x = 0; x < 4; ++x) t.out[o + 4 * x] = val;
  }
}

__device__ __forceinline__ void adam_pack_flat(const AdamPackBatch& b, const AdamPackTensor& X, const AdamConst& k,
                                               int local, int tid);

// The call's step-counter increment rides on its last launch: every block computes with
// step + 1 (read at entry), and the last block to arrive stores it -- after every block of
// every launch of the call has read the old value (no separate increment launch ahead of the
// step).  The arrival ticket is the group's own word next to its counter (step[1], 0 between
// calls), so optimizer steps of different groups / optimizers / streams never share one.

__global__ __launch_bounds__(AP_THREADS) void adam_pack_kernel(AdamPackBatch b, const double* __restrict__ hyper,
                                                               float* step, int bump) {
  __shared__ float T[32 * AP_TLD];  // brick [a][b][tap]: b stride 17, a stride 548 (4 consecutive a: distinct banks)
  int j = 0;
  while (j + 1 < b.cnt && (int)blockIdx.x >= b.first[j + 1]) ++j;
  const AdamPackTensor X = b.t[j];
  const float st1 = step[0] + 1.f;
  const AdamConst k = adam_const(hyper, &st1);
  const int local = (int)blockIdx.x - b.first[j], tid = threadIdx.x;
  if (X.brick) {
    const AdamPackT& t0 = b.pk[X.pk0];
    const int B = t0.B, a0 = 32 * (local / X.bricks_b), b0 = 32 * (local % X.bricks_b);
    {  // 32 rows of 32 b x 16 taps (2 KB contiguous each)
      float4 P[4], G[4], M[4], V[4];
      long long off[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int jj = tid + AP_THREADS * u, al = jj >> 7, f = jj & 127;
        off[u] = ((long long)(a0 + al) * B + b0) * 16 + 4 * f;
        P[u] = *reinterpret_cast<const float4*>(X.p + off[u]);
        G[u] = *reinterpret_cast<const float4*>(X.g + off[u]);
        M[u] = *reinterpret_cast<const float4*>(X.m + off[u]);
        V[u] = *reinterpret_cast<const float4*>(X.v + off[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        adam_elem(k, G[u].x, P[u].x, M[u].x, V[u].x);
        adam_elem(k, G[u].y, P[u].y, M[u].y, V[u].y);
        adam_elem(k, G[u].z, P[u].z, M[u].z, V[u].z);
        adam_elem(k, G[u].w, P[u].w, M[u].w, V[u].w);
        *reinterpret_cast<float4*>(X.m + off[u]) = M[u];
        *reinterpret_cast<float4*>(X.v + off[u]) = V[u];
        *reinterpret_cast<float4*>(X.p + off[u]) = P[u];
        const int jj = tid + AP_THREADS * u, al = jj >> 7, f = jj & 127, bl = f >> 2, tq = f & 3;
        float* d = T + al * AP_TLD + bl * 17 + 4 * tq;
        d[0] = P[u].x; d[1] = P[u].y; d[2] = P[u].z; d[3] = P[u].w;
      }
    }
    __syncthreads();
    for (int q = 0; q < X.npk; ++q) {
      const AdamPackT& t = b.pk[X.pk0 + q];
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // 32 x 16 x 8 float4 of 4 consecutive in-indices
        const int jj = tid + AP_THREADS * u, iq = jj & 7, tap = (jj >> 3) & 15, ol = jj >> 7;
        float4 v4;
        long long dst;
        if (t.in_is_a) {  // in = a: T[4 iq + c][ol][tap]
          const float* s = T + (4 * iq) * AP_TLD + ol * 17 + tap;
          v4 = make_float4(s[0], s[AP_TLD], s[2 * AP_TLD], s[3 * AP_TLD]);
          dst = apk_brick_dst(t, a0 + 4 * iq, b0 + ol, tap);
        } else {          // in = b: T[ol][4 iq + c][tap]
          const float* s = T + ol * AP_TLD + (4 * iq) * 17 + tap;
          v4 = make_float4(s[0], s[17], s[34], s[51]);
          dst = apk_brick_dst(t, a0 + ol, b0 + 4 * iq, tap);
        }
        *reinterpret_cast<float4*>(t.out + dst) = v4;
      }
    }
  } else {
    adam_pack_flat(b, X, k, local, tid);
  }
  if (bump) {
    __syncthreads();  // every wave of this block has read step[0]
    unsigned int* ticket = reinterpret_cast<unsigned int*>(step + 1);
    if (threadIdx.x == 0 && atomicAdd(ticket, 1u) == gridDim.x - 1) {
      step[0] = st1;
      atomicExch(ticket, 0u);
    }
  }
}

__device__ __forceinline__ void adam_pack_flat(const AdamPackBatch& b, const AdamPackTensor& X, const AdamConst& k,
                                               int local, int tid) {
  const long long e0 = (long long)local * AP_FLAT, e1 = min(X.n, e0 + AP_FLAT);
  const bool vec = (X.n & 3) == 0 && ((((uintptr_t)X.p | (uintptr_t)X.g | (uintptr_t)X.m | (uintptr_t)X.v) & 15) == 0);
  if (vec) {
    constexpr int U = AP_FLAT / (4 * AP_THREADS);
    float4 P[U], G[U], M[U], V[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long i = e0 + 4 * (tid + AP_THREADS * u);
      if (i < e1) {
        P[u] = *reinterpret_cast<const float4*>(X.p + i);
        G[u] = *reinterpret_cast<const float4*>(X.g + i);
        M[u] = *reinterpret_cast<const float4*>(X.m + i);
        V[u] = *reinterpret_cast<const float4*>(X.v + i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long i = e0 + 4 * (tid + AP_THREADS * u);
      if (i < e1) {
        adam_elem(k, G[u].x, P[u].x, M[u].x, V[u].x);
        adam_elem(k, G[u].y, P[u].y, M[u].y, V[u].y);
        adam_elem(k, G[u].z, P[u].z, M[u].z, V[u].z);
        adam_elem(k, G[u].w, P[u].w, M[u].w, V[u].w);
        *reinterpret_cast<float4*>(X.m + i) = M[u];
        *reinterpret_cast<float4*>(X.v + i) = V[u];
        *reinterpret_cast<float4*>(X.p + i) = P[u];
        for (int q = 0; q < X.npk; ++q) {
          const AdamPackT& t = b.pk[X.pk0 + q];
          apk_scatter(t, i, P[u].x);
          apk_scatter(t, i + 1, P[u].y);
          apk_scatter(t, i + 2, P[u].z);
          apk_scatter(t, i + 3, P[u].w);
        }
      }
    }
  } else {
    for (long long i = e0 + tid; i < e1; i += AP_THREADS) {
      float p = X.p[i], m = X.m[i], v = X.v[i];
      adam_elem(k, X.g[i], p, m, v);
      X.m[i] = m;
      X.v[i] = v;
      X.p[i] = p;
      for (int q = 0; q < X.npk; ++q) apk_scatter(b.pk[X.pk0 + q], i, p);
    }
  }
}

void launch_pack(const PackArgs& a, hipStream_t s) {
  if (pack_t2d_ok(a)) {
    pack_t2d<<<dim3(a.N / PT_N, a.K / PT_K), 256, 0, s>>>(a);
    return;
  }
  int gx, gy;
  const int kind = pack_kind(a, gx, gy);
  if (kind == 0) {
    pack_tiled16<<<dim3(gx, gy), 256, 0, s>>>(a);
    return;
  }
  if (kind == 1) {
    pack_tiled<<<dim3(gx, gy), 256, 0, s>>>(a);
    return;
  }
  const int ny = std::min(a.N, 8192);
  pack_weights<<<dim3(ceil_div(a.K, 256), ny, a.phases), 256, 0, s>>>(a);
}

void launch_pack_plan(Plan& p, float* out, hipStream_t s) {
  if (p.mode == MODE_NARROW_T) {
    launch_pack_narrow(p, out, s);
  } else {
    p.pk.out = out;
    launch_pack(p.pk, s);
  }
}

}  // namespace rgan

using namespace rgan;

extern "C" size_t rgan_conv_pack_floats(const RganConv* d, int which) {
  Plan p;
  const int rc = plan_placeholder(d, which, nullptr, p);
  if (rc || which > 1 || !p.pack) return 0;  // 0: no packed layout (or unsupported)
  return p.pack_floats;
}

extern "C" int rgan_conv_pack(const RganConv* d, int which, const float* w, float* packed, void* stream) {
  if (!w || !packed || which < 0 || which > 1) return RGAN_EINVAL;
  Plan p;
  int rc = plan_placeholder(d, which, w, p);
  if (rc) return rc;
  if (!p.pack) return RGAN_EINVAL;
  launch_pack_plan(p, packed, (hipStream_t)stream);
  RGAN_CHECK_LAUNCH();
  return 0;
}

extern "C" int rgan_conv_pack_batch(int n, const RganConv* const* d, const int* which, const float* const* w,
                                    float* const* packed, void* stream) {
  if (n < 0 || (n > 0 && (!d || !which || !w || !packed))) return RGAN_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  PackBatch b{};
  long long blocks = 0;
  auto flush = [&]() {
    if (b.n == 0) return;
    b.first[b.n] = (int)blocks;
    pack_multi<<<(unsigned)blocks, 256, 0, s>>>(b);
    b = PackBatch{};
    blocks = 0;
  };
  for (int i = 0; i < n; ++i) {
    if (!w[i] || !packed[i] || which[i] < 0 || which[i] > 1) return RGAN_EINVAL;
    Plan p;
    const int rc = plan_placeholder(d[i], which[i], w[i], p);
    if (rc) return rc;
    if (!p.pack) return RGAN_EINVAL;
    int gx = 0, gy = 0;
    const int kind = p.mode == MODE_NARROW_T ? -1 : (p.pk.out = packed[i], pack_kind(p.pk, gx, gy));
    if (kind < 0) {  // narrow / generic layouts: their own launch
      launch_pack_plan(p, packed[i], s);
      RGAN_CHECK_LAUNCH();
      continue;
    }
    if (b.n == PACK_BATCH || blocks + (long long)gx * gy >= (1LL << 30)) flush();
    b.a[b.n] = p.pk;
    b.kind[b.n] = kind;
    b.gx[b.n] = gx;
    b.first[b.n] = (int)blocks;
    blocks += (long long)gx * gy;
    ++b.n;
  }
  flush();
  RGAN_CHECK_LAUNCH();
  return 0;
}

extern "C" int rgan_adam_packed(int ntensors, float* const* params, const float* const* grads,
                                float* const* exp_avg, float* const* exp_avg_sq, const long long* numel,
                                const double* hyper, float* step, int npacks, const RganAdamPack* packs,
                                void* stream) {
  RGAN_REQUIRE(ntensors >= 0 && npacks >= 0 && hyper && step && (npacks == 0 || packs));
  RGAN_REQUIRE(ntensors == 0 || (params && grads && exp_avg && exp_avg_sq && numel));
  hipStream_t s = (hipStream_t)stream;
  for (int j = 0; j < ntensors; ++j)
    RGAN_REQUIRE(params[j] && grads[j] && exp_avg[j] && exp_avg_sq[j] && numel[j] >= 0 && numel[j] < (1LL << 31));
  // plan every layout: in-kernel (AdamPackT) or a repack launch after the step
  std::vector<std::vector<AdamPackT>> per(ntensors);
  std::vector<Plan> later;
  std::vector<float*> later_out;
  for (int i = 0; i < npacks; ++i) {
    const RganAdamPack& q = packs[i];
    RGAN_REQUIRE(q.d && q.packed && q.tensor >= 0 && q.tensor < ntensors && (q.which == 0 || q.which == 1));
    Plan p;
    const float* W = params[q.tensor];
    const int rc = plan_placeholder(q.d, q.which, W, p);
    if (rc) return rc;
    RGAN_REQUIRE(p.pack);
    const long long n = numel[q.tensor];
    AdamPackT t{};
    t.out = q.packed;
    bool ok = false;
    const PackArgs& a = p.pk;
    if (p.mode == MODE_NARROW_T) {
      const int C = p.na.C, NC = p.na.Cout;
      ok = p.pn_s_out == 16 && p.pn_s_in == 16LL * NC && (long long)C * NC * 16 == n;
      t.kind = APK_NARROW; t.A = C; t.B = NC; t.KK = 16;
    } else if (pack_t2d_ok(a)) {
      const int T = a.KH * a.KW, Cout = (int)a.fnco.d;
      ok = (long long)a.K * Cout * T == n;
      t.kind = APK_T2D; t.A = a.K; t.B = Cout; t.KK = T; t.K = a.K;
      t.in_is_a = 1;  // k = ci = the weight's first index: runs of 4 consecutive ci
    } else {
      int gx, gy;
      const int kind = pack_kind(a, gx, gy);
      const int KK = a.KH * a.KW, Nin = (int)a.fpci.d, Nout = a.N;
      if (kind >= 0 && a.s_kw == 1 && a.s_kh == a.KW && (long long)Nin * Nout * KK == n) {
        t.kind = APK_TILED; t.KK = KK; t.KW = a.KW; t.flip = a.flip; t.convt2 = a.convt2;
        t.Nin = Nin; t.Nout = Nout; t.K = a.K;
        if (a.s_in == KK && a.s_out == (long long)Nin * KK) {         // in = second index
          ok = true; t.in_is_a = 0; t.A = Nout; t.B = Nin;
        } else if (a.s_out == KK && a.s_in == (long long)Nout * KK) {  // in = first index
          ok = true; t.in_is_a = 1; t.A = Nin; t.B = Nout;
        }
      }
    }
    if (ok) {
      per[q.tensor].push_back(t);
    } else {
      later.push_back(p);
      later_out.push_back(q.packed);
    }
  }
  RGAN_CHECK_LAUNCH();
  AdamPackBatch b{};
  long long blocks = 0;
  int np = 0;
  bool bumped = false;
  auto flush = [&](bool last) -> int {
    if (b.cnt == 0) return 0;
    b.first[b.cnt] = (int)blocks;
    if (blocks > 0) {
      adam_pack_kernel<<<(unsigned)blocks, AP_THREADS, 0, s>>>(b, hyper, step, last ? 1 : 0);
      bumped = last;
    }
    RGAN_CHECK_LAUNCH();
    b = AdamPackBatch{};
    blocks = 0;
    np = 0;
    return 0;
  };
  for (int j = 0; j < ntensors; ++j) {
    auto& L = per[j];
    const int nt = (int)L.size();
    RGAN_REQUIRE(nt <= AP_MAXP);
    if (b.cnt == AP_MAXT || np + nt > AP_MAXP) {
      const int rc = flush(false);
      if (rc) return rc;
    }
    AdamPackTensor X{params[j], grads[j], exp_avg[j], exp_avg_sq[j], numel[j], 0, 0, np, nt};
    bool brick = nt > 0 && ((((uintptr_t)params[j] | (uintptr_t)grads[j] | (uintptr_t)exp_avg[j] |
                               (uintptr_t)exp_avg_sq[j]) & 15) == 0);
    for (const auto& t : L) {
      brick = brick && (t.kind == APK_TILED || t.kind == APK_T2D) && t.KK == 16 && t.A == L[0].A &&
              t.B == L[0].B && t.A % 32 == 0 && t.B % 32 == 0 && aligned16(t.out);
      b.pk[np++] = t;
    }
    X.brick = brick;
    X.bricks_b = brick ? L[0].B / 32 : 0;
    const long long nb = brick ? (long long)(L[0].A / 32) * (L[0].B / 32) : (numel[j] + AP_FLAT - 1) / AP_FLAT;
    b.t[b.cnt] = X;
    b.first[b.cnt] = (int)blocks;
    blocks += nb;
    RGAN_REQUIRE(blocks < (1LL << 30));
    ++b.cnt;
  }
  int rc = flush(true);
  if (rc) return rc;
  if (!bumped) {  // no block ran the last launch's ticket: a separate increment
    rc = rgan_adam_step_inc(step, stream);
    if (rc) return rc;
  }
  for (size_t i = 0; i < later.size(); ++i) {  // layouts the kernel does not write: repack
    launch_pack_plan(later[i], later_out[i], s);
    RGAN_CHECK_LAUNCH();
  }
  return 0;
}
