// Nearest training images and k-NN precision / recall in pixel space for gfx950 (--rgan_nn_every,
// evaluate --rgan_nn; Kynkaanniemi et al., "Improved Precision and Recall Metric for Assessing
// Generative Models", NeurIPS 2019; DESIGN "Nearest training images").  Everything is integer:
//
//   nn_pack_u8   u8 images through element strides -> int8 descriptor rows (rounded f x f box mean,
//                minus 128, zero pad to a multiple of 64 bytes) and their int32 squared norms
//   nn_dist<E>   d2[q][r] = na[q] + nb[r] - 2 a[q].b[r] by v_mfma_i32_32x32x32_i8 from LDS tiles, the
//                epilogue E consuming each d2 in registers: TopK keeps a lane's 8 smallest keys
//                (uint64(d2) << 32 | r), Covered ORs d2 <= radius[r]
//   nn_merge     the parts' keys of a query -> its k smallest, as dist / idx
//
// Tiling of nn_dist: a block of 4 waves owns 128 queries and one contiguous part of the references,
// which it walks in steps of 128; a wave owns 64 queries x 64 references of a step, four 32x32 i32
// accumulators.  The references go in as the A operand and the queries as the B operand, so a
// result's column (the lane) is a query and its rows (the 16 registers) are references: a lane keeps
// the running best of its two queries in registers and no lane talks to another before the end of the
// part, where the two lane halves and the two waves that share a query are merged through LDS.
// K runs through LDS in chunks of 128 bytes: image [row][8 slots of 16 B], slot s of row r stored at
// slot s ^ ((r >> 1) & 7), so the 16 rows a ds_read_b128 quarter-wave reads fall on 16 different bank
// groups; the next chunk is in flight in registers while the MFMAs of this one run.
// Both operands take their 16 bytes of a 32-byte k step from the same slot (2 step + lane half), so the
// products pair equal k whatever order the instruction gives the bytes inside a lane.
//
// No float, no atomics: keys are distinct (r is part of the key), so the k smallest are a function of
// the inputs alone, whatever the step, the part or the order of the merges.
#include <limits.h>

#include "common.h"

namespace rgan {

using v4i = __attribute__((ext_vector_type(4))) int;
using v16i = __attribute__((ext_vector_type(16))) int;

constexpr int NN_T = 128;                     // queries per block; references per step
constexpr int NN_BK = 128;                    // bytes of K per LDS chunk
constexpr int NN_TILE = NN_T * NN_BK;         // bytes of one operand's LDS image
constexpr int NN_KEEP = 8;                    // keys a lane keeps per query (k <= 8)
constexpr uint64_t NN_NONE = ~(uint64_t)0;    // no key: above every (d2 << 32 | r), d2 < 2^31

// best[] ascending; key takes its place if it is below best[7]
__device__ __forceinline__ void keep_insert(uint64_t (&best)[NN_KEEP], uint64_t key) {
  if (key >= best[NN_KEEP - 1]) return;
#pragma unroll
  for (int i = NN_KEEP - 1; i > 0; --i)
    if (key < best[i]) best[i] = key < best[i - 1] ? best[i - 1] : key;
  if (key < best[0]) best[0] = key;
}

__device__ __forceinline__ int lds_off(int row, int slot) { return row * NN_BK + ((slot ^ ((row >> 1) & 7)) << 4); }

struct TopKArgs {
  uint64_t* part;  // [Q][nsplit][k]
  int k;
};

struct TopK {
  using Args = TopKArgs;
  uint64_t best[2][NN_KEEP];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < NN_KEEP; ++j) best[i][j] = NN_NONE;
  }
  __device__ __forceinline__ void visit(int qi, int d2, int r, const Args&) {
    keep_insert(best[qi], ((uint64_t)(uint32_t)d2 << 32) | (uint32_t)r);
  }
  // lds: 32 KB, free to use after the caller's barrier.  keys[list][j][query]: list = 2 wr + lane half
  __device__ __forceinline__ void finish(unsigned char* lds, int q0, int Q, int part, int nsplit, int wq, int wr,
                                         int col, int h, const Args& args) {
    uint64_t* keys = reinterpret_cast<uint64_t*>(lds);
#pragma unroll
    for (int qi = 0; qi < 2; ++qi)
#pragma unroll
      for (int j = 0; j < NN_KEEP; ++j)
        keys[((2 * wr + h) * NN_KEEP + j) * NN_T + wq * 64 + qi * 32 + col] = best[qi][j];
    __syncthreads();
    const int t = threadIdx.x, q = q0 + t;
    if (t >= NN_T || q >= Q) return;
    uint64_t m[NN_KEEP];
#pragma unroll
    for (int j = 0; j < NN_KEEP; ++j) m[j] = keys[j * NN_T + t];
    for (int i = NN_KEEP; i < 4 * NN_KEEP; ++i) keep_insert(m, keys[i * NN_T + t]);
    uint64_t* out = args.part + ((long long)q * nsplit + part) * args.k;
#pragma unroll
    for (int j = 0; j < NN_KEEP; ++j)
      if (j < args.k) out[j] = m[j];
  }
};

struct CoveredArgs {
  const int* radius;  // [R]
  int* flag;          // [Q], zeroed before the launch
};

struct Covered {
  using Args = CoveredArgs;
  int found[2];
  __device__ __forceinline__ void init() { found[0] = found[1] = 0; }
  __device__ __forceinline__ void visit(int qi, int d2, int r, const Args& args) { found[qi] |= d2 <= args.radius[r]; }
  __device__ __forceinline__ void finish(unsigned char* lds, int q0, int Q, int, int, int wq, int, int col, int,
                                         const Args& args) {
    int* any = reinterpret_cast<int*>(lds);
    if (threadIdx.x < NN_T) any[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int qi = 0; qi < 2; ++qi)
      if (found[qi]) any[wq * 64 + qi * 32 + col] = 1;  // every writer stores the same 1
    __syncthreads();
    const int t = threadIdx.x, q = q0 + t;
    if (t < NN_T && q < Q && any[t]) args.flag[q] = 1;  // so does every part's block
  }
};

template <class Epi>
__global__ __launch_bounds__(256) void nn_dist(const int8_t* __restrict__ a, const int* __restrict__ na, int Q,
                                               const int8_t* __restrict__ b, const int* __restrict__ nb, int R,
                                               int row_bytes, long long self_offset, int nsplit,
                                               typename Epi::Args args) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * NN_TILE];
  unsigned char* lds_ref = lds;             // A operand: references
  unsigned char* lds_qry = lds + NN_TILE;   // B operand: queries
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wq = wave & 1, wr = wave >> 1, col = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * NN_T, part = blockIdx.y;
  const int rbeg = (int)((long long)part * R / nsplit), rend = (int)((long long)(part + 1) * R / nsplit);

  Epi epi;
  epi.init();
  int qrow[2], qnorm[2];
#pragma unroll
  for (int qi = 0; qi < 2; ++qi) {
    qrow[qi] = q0 + wq * 64 + qi * 32 + col;
    qnorm[qi] = qrow[qi] < Q ? na[qrow[qi]] : 0;
  }

  for (int r0 = rbeg; r0 < rend; r0 += NN_T) {
    v16i acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;

    // staging: 16-byte piece i of a thread is row (tid + 256 i) >> 3, slot (tid + 256 i) & 7 of a chunk
    uint4 sref[4], sqry[4];
    auto fetch = [&](int k0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = tid + 256 * i, row = p >> 3, kb = k0 + ((p & 7) << 4);
        const int r = r0 + row, q = q0 + row;
        sref[i] = make_uint4(0u, 0u, 0u, 0u);
        sqry[i] = make_uint4(0u, 0u, 0u, 0u);
        if (kb < row_bytes) {
          if (r < rend) sref[i] = *reinterpret_cast<const uint4*>(b + (long long)r * row_bytes + kb);
          if (q < Q) sqry[i] = *reinterpret_cast<const uint4*>(a + (long long)q * row_bytes + kb);
        }
      }
    };
    fetch(0);
    for (int k0 = 0; k0 < row_bytes; k0 += NN_BK) {
      __syncthreads();  // the previous chunk's (or the last part epilogue's) reads of the LDS are done
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = tid + 256 * i, off = lds_off(p >> 3, p & 7);
        *reinterpret_cast<uint4*>(lds_ref + off) = sref[i];
        *reinterpret_cast<uint4*>(lds_qry + off) = sqry[i];
      }
      __syncthreads();
      if (k0 + NN_BK < row_bytes) fetch(k0 + NN_BK);
#pragma unroll
      for (int ks = 0; ks < NN_BK / 32; ++ks) {
        v4i fr[2], fq[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          fr[i] = *reinterpret_cast<const v4i*>(lds_ref + lds_off(wr * 64 + i * 32 + col, 2 * ks + h));
          fq[i] = *reinterpret_cast<const v4i*>(lds_qry + lds_off(wq * 64 + i * 32 + col, 2 * ks + h));
        }
#pragma unroll
        for (int qi = 0; qi < 2; ++qi)
#pragma unroll
          for (int ri = 0; ri < 2; ++ri)
            acc[qi][ri] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fr[ri], fq[qi], acc[qi][ri], 0, 0, 0);
      }
    }

    // result (ri, e) of a lane: reference row (e & 3) + 8 (e >> 2) + 4 h of its 32, query = the lane's column
#pragma unroll
    for (int ri = 0; ri < 2; ++ri)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = r0 + wr * 64 + ri * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (r >= rend) continue;
        const int rn = nb[r];
#pragma unroll
        for (int qi = 0; qi < 2; ++qi) {
          if (qrow[qi] >= Q || (long long)(r - qrow[qi]) == self_offset) continue;
          epi.visit(qi, qnorm[qi] + rn - 2 * acc[qi][ri][e], r, args);
        }
      }
  }
  __syncthreads();  // the tiles are read: the LDS is the epilogue's
  epi.finish(lds, q0, Q, part, nsplit, wq, wr, col, h, args);
}

// One thread per query: the nsplit k keys of its parts -> its k smallest.
__global__ __launch_bounds__(256) void nn_merge(const uint64_t* __restrict__ part, int Q, int nsplit, int k,
                                                int* __restrict__ dist, int* __restrict__ idx) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  uint64_t m[NN_KEEP];
#pragma unroll
  for (int j = 0; j < NN_KEEP; ++j) m[j] = NN_NONE;
  const uint64_t* keys = part + (long long)q * nsplit * k;
  for (int i = 0; i < nsplit * k; ++i) keep_insert(m, keys[i]);
#pragma unroll
  for (int j = 0; j < NN_KEEP; ++j)
    if (j < k) {
      const bool none = m[j] == NN_NONE;
      dist[(long long)q * k + j] = none ? INT_MAX : (int)(uint32_t)(m[j] >> 32);
      idx[(long long)q * k + j] = none ? -1 : (int)(uint32_t)m[j];
    }
}

// One block per image.  The box sum is at most 255 * 32 * 32 and the norm at most 128^2 * 12288: int.
__global__ __launch_bounds__(256) void nn_pack_u8(const uint8_t* __restrict__ in, int C, int S, long long sn,
                                                  long long sc, long long sh, long long sw, int s, int row_bytes,
                                                  int8_t* __restrict__ desc, int* __restrict__ norm) {
  __shared__ int red[4];
  const int n = blockIdx.x, f = S / s, D = C * s * s, ff = f * f;
  const uint8_t* img = in + n * sn;
  int8_t* row = desc + (long long)n * row_bytes;
  int sq = 0;
  for (int i = threadIdx.x; i < row_bytes; i += 256) {
    int v = 0;
    if (i < D) {
      const int x = i % s, y = (i / s) % s, c = i / (s * s);
      const uint8_t* box = img + c * sc + (long long)(y * f) * sh + (long long)(x * f) * sw;
      int sum = 0;
      for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) sum += box[dy * sh + dx * sw];
      v = (sum + ff / 2) / ff - 128;
    }
    row[i] = (int8_t)v;
    sq += v * v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) norm[n] = red[0] + red[1] + red[2] + red[3];
}

}  // namespace rgan

using namespace rgan;

static const int kMaxSplits = 4096;
static const long long kMaxStride = (1ll << 40);

static bool side_ok(int s) { return s == 8 || s == 16 || s == 32 || s == 64; }
static bool row_ok(int row_bytes) { return row_bytes >= 64 && row_bytes % 64 == 0 && row_bytes <= RGAN_NN_MAX_ROW_BYTES; }
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// what a self_offset can match is r - q in [-(Q - 1), R - 1]; everything else excludes nothing
static int steps_of(int n, int per) { return (int)(((long long)n + per - 1) / per); }
static long long self_or_none(long long self_offset, int Q, int R) {
  return (self_offset < -(long long)Q || self_offset > (long long)R) ? RGAN_NN_NO_SELF : self_offset;
}

extern "C" size_t rgan_nn_row_bytes(int C, int s) {
  if (C < 1 || C > 4 || !side_ok(s)) return 0;
  const size_t bytes = ((size_t)C * s * s + 63) / 64 * 64;
  return bytes > RGAN_NN_MAX_ROW_BYTES ? 0 : bytes;
}

extern "C" int rgan_nn_pack_u8(const uint8_t* in, int N, int C, int S, const long long* strides, int s, int8_t* desc,
                               int* norm, void* stream) {
  RGAN_REQUIRE(in && strides && desc && norm);
  RGAN_REQUIRE(N >= 1 && S >= 1);
  const size_t row_bytes = rgan_nn_row_bytes(C, s);
  RGAN_REQUIRE(row_bytes > 0);
  RGAN_REQUIRE(S % s == 0 && S / s <= 32);
  for (int i = 0; i < 4; ++i) RGAN_REQUIRE(strides[i] >= 0 && strides[i] <= kMaxStride);
  nn_pack_u8<<<(unsigned)N, 256, 0, (hipStream_t)stream>>>(in, C, S, strides[0], strides[1], strides[2], strides[3], s,
                                                           (int)row_bytes, desc, norm);
  RGAN_CHECK_LAUNCH();
  return 0;
}

// Enough blocks for two per compute unit (256 of them), a part no shorter than one step of 128 rows.
extern "C" int rgan_nn_topk_splits(int Q, int R) {
  if (Q < 1 || R < 1) return 0;
  const int qblocks = steps_of(Q, NN_T), steps = steps_of(R, NN_T);
  int n = (512 + qblocks - 1) / qblocks;
  if (n > steps) n = steps;
  if (n > kMaxSplits) n = kMaxSplits;
  return n < 1 ? 1 : n;
}

// the number of parts a call uses, or 0 when its sizes are refused
static int splits_for(int Q, int R, int k, int nsplit) {
  if (Q < 1 || R < 1 || k < 1 || k > NN_KEEP || nsplit < 0 || nsplit > kMaxSplits) return 0;
  const int ns = nsplit ? nsplit : rgan_nn_topk_splits(Q, R);
  if ((long long)Q * ns * k > INT_MAX) return 0;
  return ns;
}

extern "C" size_t rgan_nn_topk_ws_bytes(int Q, int R, int k, int nsplit) {
  const int ns = splits_for(Q, R, k, nsplit);
  return ns ? (size_t)Q * ns * k * sizeof(uint64_t) : 0;
}

extern "C" int rgan_nn_topk(const int8_t* a, const int* na, int Q, const int8_t* b, const int* nb, int R,
                            int row_bytes, int k, long long self_offset, int nsplit, int* dist, int* idx, void* ws,
                            size_t ws_bytes, void* stream) {
  RGAN_REQUIRE(a && na && b && nb && dist && idx && ws);
  RGAN_REQUIRE(row_ok(row_bytes));
  const int ns = splits_for(Q, R, k, nsplit);
  RGAN_REQUIRE(ns > 0);
  RGAN_REQUIRE(ws_bytes >= rgan_nn_topk_ws_bytes(Q, R, k, nsplit));
  RGAN_REQUIRE(aligned16(a) && aligned16(b) && ((uintptr_t)ws & 7) == 0);
  const dim3 grid((unsigned)steps_of(Q, NN_T), (unsigned)ns);
  const TopKArgs args = {(uint64_t*)ws, k};
  nn_dist<TopK><<<grid, 256, 0, (hipStream_t)stream>>>(a, na, Q, b, nb, R, row_bytes, self_or_none(self_offset, Q, R),
                                                       ns, args);
  nn_merge<<<(unsigned)steps_of(Q, 256), 256, 0, (hipStream_t)stream>>>((const uint64_t*)ws, Q, ns, k, dist, idx);
  RGAN_CHECK_LAUNCH();
  return 0;
}

extern "C" int rgan_nn_covered(const int8_t* a, const int* na, int Q, const int8_t* b, const int* nb,
                               const int* radius, int R, int row_bytes, long long self_offset, int* flag,
                               void* stream) {
  RGAN_REQUIRE(a && na && b && nb && radius && flag);
  RGAN_REQUIRE(Q >= 1 && R >= 1 && row_ok(row_bytes));
  RGAN_REQUIRE(aligned16(a) && aligned16(b));
  const int ns = rgan_nn_topk_splits(Q, R);
  const dim3 grid((unsigned)steps_of(Q, NN_T), (unsigned)ns);
  const CoveredArgs args = {radius, flag};
  if (hipMemsetAsync(flag, 0, (size_t)Q * sizeof(int), (hipStream_t)stream) != hipSuccess) return (int)hipGetLastError();
  nn_dist<Covered><<<grid, 256, 0, (hipStream_t)stream>>>(a, na, Q, b, nb, R, row_bytes,
                                                          self_or_none(self_offset, Q, R), ns, args);
  RGAN_CHECK_LAUNCH();
  return 0;
}
