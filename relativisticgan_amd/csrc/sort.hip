// Segmented key sort for gfx950: nseg contiguous segments of len fp32 keys each, ascending, keys
// only (the sliced Wasserstein metric's sort, swd.hip; the library's first general device
// primitive).  No rocPRIM / hipCUB: a least-significant-digit radix sort, 4 passes of 8 bits.
//
// Order: the usual total order of the bit patterns, key(u) = u ^ (u >> 31 ? 0xffffffff :
// 0x80000000) compared as uint32: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN, NaN patterns by
// their bits.  The stored values are the input's own bits (the map is applied to read a digit only).
//
// One pass (digit = bits [8 pass, 8 pass + 8) of the key), over tiles of SORT_TILE = 2048 keys, a
// segment's tiles numbered b < nblk = ceil(len / SORT_TILE), the last one possibly short:
//   1. sort_hist:    hist[seg][digit][b] = this tile's count of the digit (integer LDS atomics);
//   2. sort_scan:    one block per segment turns hist[seg] into its exclusive prefix sum in
//                    (digit, b) order: where tile b's keys of a digit go in the segment;
//   3. sort_scatter: a STABLE scatter.  A tile's keys are taken in rounds of 256 (key j 256 + t by
//                    thread t), so input order is (round, wave, lane).  Each wave finds the lanes
//                    that hold its digit with eight __ballot's (wave64: 64-bit masks); a key's rank
//                    among them is the popcount of the lower lanes, the first lane of each group
//                    stores the group's size into cnt[round 4 + wave][digit] (one writer per cell),
//                    thread d scans cnt[.][d] over the 32 (round, wave) rows in order, and a key goes
//                    to hist[seg][digit][b] + cnt[row][digit] + rank.  No rank depends on the order
//                    in which atomics arrive, so equal inputs give equal outputs and each pass keeps
//                    the order of equal digits, which is what makes LSD passes compose.
// Passes ping-pong in -> tmp -> out -> tmp -> out.  Algorithmic traffic: 3 x 4 B per key and pass
// (histogram read, scatter read and write), 48 B per key in all, plus the 1 KiB histogram per tile.
#include "common.h"

namespace rgan {

constexpr int SORT_THREADS = 256;
constexpr int SORT_ROUNDS = 8;
constexpr int SORT_TILE = SORT_THREADS * SORT_ROUNDS;  // 2048 keys per block
constexpr int SORT_ROWS = SORT_ROUNDS * (SORT_THREADS / 64);

__device__ __forceinline__ uint32_t sort_digit(uint32_t u, int shift) {
  const uint32_t key = u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
  return (key >> shift) & 255u;
}

// grid: nseg * nblk blocks; block g: segment g / nblk, tile g % nblk
__global__ __launch_bounds__(SORT_THREADS) void sort_hist(const uint32_t* __restrict__ in, int len, int nblk,
                                                          int shift, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  const int seg = blockIdx.x / nblk, b = blockIdx.x % nblk;
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t* src = in + (long long)seg * len;
  const int lo = b * SORT_TILE;
#pragma unroll
  for (int j = 0; j < SORT_ROUNDS; ++j) {
    const int i = lo + j * SORT_THREADS + threadIdx.x;
    if (i < len) atomicAdd(&h[sort_digit(src[i], shift)], 1u);
  }
  __syncthreads();
  hist[((long long)seg * 256 + threadIdx.x) * nblk + b] = h[threadIdx.x];
}

// grid: nseg blocks; exclusive prefix sum of hist[seg][0 .. 256 nblk) in place
__global__ __launch_bounds__(SORT_THREADS) void sort_scan(uint32_t* __restrict__ hist, int nblk) {
  __shared__ uint32_t total[256];
  uint32_t* h = hist + (long long)blockIdx.x * 256 * nblk;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // a digit's total: wave `wave` owns digits wave, wave + 4, ...
  for (int d = wave; d < 256; d += 4) {
    uint32_t s = 0;
    for (int i = lane; i < nblk; i += 64) s += h[(long long)d * nblk + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) total[d] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int d = 0; d < 256; ++d) {
      const uint32_t t = total[d];
      total[d] = run;
      run += t;
    }
  }
  __syncthreads();
  for (int d = wave; d < 256; d += 4) {
    uint32_t carry = total[d];
    for (int i0 = 0; i0 < nblk; i0 += 64) {
      const int i = i0 + lane;
      const uint32_t v = i < nblk ? h[(long long)d * nblk + i] : 0u;
      uint32_t inc = v;  // inclusive scan over the wave
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
      }
      if (i < nblk) h[(long long)d * nblk + i] = carry + inc - v;
      carry += __shfl(inc, 63, 64);
    }
  }
}

__global__ __launch_bounds__(SORT_THREADS) void sort_scatter(const uint32_t* __restrict__ in,
                                                             uint32_t* __restrict__ out, int len, int nblk, int shift,
                                                             const uint32_t* __restrict__ hist) {
  __shared__ uint32_t cnt[SORT_ROWS][256];
  const int seg = blockIdx.x / nblk, b = blockIdx.x % nblk;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t* src = in + (long long)seg * len;
  uint32_t* dst = out + (long long)seg * len;
  const int lo = b * SORT_TILE;
#pragma unroll
  for (int r = 0; r < SORT_ROWS; ++r) cnt[r][threadIdx.x] = 0;
  __syncthreads();
  uint32_t key[SORT_ROUNDS], rank[SORT_ROUNDS];
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < SORT_ROUNDS; ++j) {
    const int i = lo + j * SORT_THREADS + threadIdx.x;
    const bool valid = i < len;
    key[j] = valid ? src[i] : 0u;
    const uint32_t d = sort_digit(key[j], shift);
    unsigned long long same = __ballot(valid);  // the lanes of this wave that hold my digit
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1u;
      const unsigned long long m = __ballot(on);
      same &= on ? m : ~m;
    }
    rank[j] = (uint32_t)__popcll(same & below);
    if (valid && rank[j] == 0) cnt[j * 4 + wave][d] = (uint32_t)__popcll(same);
  }
  __syncthreads();
  {  // thread d: exclusive scan of digit d's counts over the (round, wave) rows, from the tile's base
    uint32_t run = hist[((long long)seg * 256 + threadIdx.x) * nblk + b];
#pragma unroll
    for (int r = 0; r < SORT_ROWS; ++r) {
      const uint32_t c = cnt[r][threadIdx.x];
      cnt[r][threadIdx.x] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < SORT_ROUNDS; ++j) {
    const int i = lo + j * SORT_THREADS + threadIdx.x;
    if (i < len) {
      const uint32_t at = cnt[j * 4 + wave][sort_digit(key[j], shift)] + rank[j];
      if (at < (uint32_t)len) dst[at] = key[j];  // (always: the offsets are a permutation of [0, len))
    }
  }
}

}  // namespace rgan

using namespace rgan;

extern "C" int rgan_sort_segments_tile(void) { return SORT_TILE; }

static bool sort_sizes_ok(int nseg, int len) {
  return nseg > 0 && len > 0 && (long long)nseg * (long long)len < (1ll << 31);
}

extern "C" size_t rgan_sort_segments_ws_bytes(int nseg, int len) {
  if (!sort_sizes_ok(nseg, len)) return 0;
  const long long nblk = ((long long)len + SORT_TILE - 1) / SORT_TILE;
  return (size_t)((long long)nseg * nblk * 256ll * (long long)sizeof(uint32_t));
}

extern "C" int rgan_sort_segments(const float* in, float* out, float* tmp, int nseg, int len, void* ws,
                                  size_t ws_bytes, void* stream) {
  RGAN_REQUIRE(in && out && tmp && ws);
  RGAN_REQUIRE(sort_sizes_ok(nseg, len));
  RGAN_REQUIRE(tmp != out && tmp != in);
  RGAN_REQUIRE(ws_bytes >= rgan_sort_segments_ws_bytes(nseg, len));
  const int nblk = (int)(((long long)len + SORT_TILE - 1) / SORT_TILE);
  const unsigned grid = (unsigned)((long long)nseg * nblk);  // <= nseg * len < 2^31
  hipStream_t s = (hipStream_t)stream;
  uint32_t* hist = (uint32_t*)ws;
  const uint32_t* src = (const uint32_t*)in;
  for (int pass = 0; pass < 4; ++pass) {
    uint32_t* dst = (uint32_t*)((pass & 1) ? out : tmp);
    sort_hist<<<grid, SORT_THREADS, 0, s>>>(src, len, nblk, 8 * pass, hist);
    sort_scan<<<(unsigned)nseg, SORT_THREADS, 0, s>>>(hist, nblk);
    sort_scatter<<<grid, SORT_THREADS, 0, s>>>(src, dst, len, nblk, 8 * pass, hist);
    src = dst;
  }
  RGAN_CHECK_LAUNCH();
  return 0;
}
