// Host-side argument checks of the rgan_swd_ entry points and rgan_sort_segments under
// AddressSanitizer + UBSan, CPU only (a stand-alone companion of abi_fuzz.cpp and lecam_args.cpp).
//
// Built by tests/test_swd_cpu.py from csrc/swd.hip and csrc/sort.hip with
// -fsanitize=address,undefined on the host half only (hipcc -Xarch_host; the device half is compiled
// normally and never launched).  Every call here is malformed in at least one argument and must
// answer RGAN_EINVAL before any launch (a launch attempt on this GPU-less host would return a HIP
// error instead, reported as a failure); the sizes sweep the integer extremes, and the workspace-size
// functions are called over all of them (a signed overflow there is a UBSan report).
//
// Exit 0 and one "swd_args ok" line, or a sanitizer report / a list of failures.
#include <cstdio>
#include <vector>

#include "rgan.h"

static int g_fail = 0;
static long long g_calls = 0;

static void expect_einval(int rc, const char* what) {
  ++g_calls;
  if (rc != RGAN_EINVAL) {
    std::fprintf(stderr, "FAIL %s: rc %d (want RGAN_EINVAL %d)\n", what, rc, RGAN_EINVAL);
    ++g_fail;
  }
}

static void expect(bool ok, const char* what) {
  ++g_calls;
  if (!ok) {
    std::fprintf(stderr, "FAIL %s\n", what);
    ++g_fail;
  }
}

static const std::vector<int> kInts = {-2147483647 - 1, -65536, -7, -1, 0, 1, 2, 3, 6, 7, 16, 31, 32, 33, 48, 63, 64,
                                       65, 255, 256, 257, 1025, 65535, 65536, 1 << 20, 1 << 28, 2147483647};

static bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

int main() {
  // dummies: never dereferenced on the host, and no call below may reach the device
  const uint8_t* u8 = reinterpret_cast<const uint8_t*>(0x1000);
  float* a = reinterpret_cast<float*>(0x2000);
  float* b = reinterpret_cast<float*>(0x3000);
  float* c = reinterpret_cast<float*>(0x4000);
  int* pos = reinterpret_cast<int*>(0x5000);
  double* dd = reinterpret_cast<double*>(0x6000);
  double* st = reinterpret_cast<double*>(0x7000);
  void* ws = reinterpret_cast<void*>(0x8000);
  const long long chw[4] = {3 * 32 * 32, 32 * 32, 32, 1};
  const long long bad[4] = {3 * 32 * 32, -1, 32, 1};
  const size_t big = ~(size_t)0;

  // ---- null pointers, sizes valid
  expect_einval(rgan_swd_load_u8(nullptr, 2, 3, 32, chw, a, nullptr), "load_u8 in");
  expect_einval(rgan_swd_load_u8(u8, 2, 3, 32, nullptr, a, nullptr), "load_u8 strides");
  expect_einval(rgan_swd_load_u8(u8, 2, 3, 32, chw, nullptr, nullptr), "load_u8 out");
  expect_einval(rgan_swd_load_u8(u8, 2, 3, 32, bad, a, nullptr), "load_u8 negative stride");
  expect_einval(rgan_swd_pyr_down(nullptr, 2, 3, 32, b, nullptr), "pyr_down in");
  expect_einval(rgan_swd_pyr_down(a, 2, 3, 32, nullptr, nullptr), "pyr_down out");
  expect_einval(rgan_swd_pyr_down(a, 2, 3, 32, a, nullptr), "pyr_down in place");
  expect_einval(rgan_swd_laplace(nullptr, b, 2, 3, 32, c, nullptr), "laplace fine");
  expect_einval(rgan_swd_laplace(a, nullptr, 2, 3, 32, c, nullptr), "laplace coarse");
  expect_einval(rgan_swd_laplace(a, b, 2, 3, 32, nullptr, nullptr), "laplace out");
  expect_einval(rgan_swd_laplace(a, b, 2, 3, 32, b, nullptr), "laplace out == coarse");
  expect_einval(rgan_swd_positions(nullptr, 8, 32, pos, nullptr), "positions u");
  expect_einval(rgan_swd_positions(a, 8, 32, nullptr, nullptr), "positions pos");
  expect_einval(rgan_swd_descriptors(nullptr, 2, 3, 32, 4, pos, b, dd, nullptr), "descriptors img");
  expect_einval(rgan_swd_descriptors(a, 2, 3, 32, 4, nullptr, b, dd, nullptr), "descriptors pos");
  expect_einval(rgan_swd_descriptors(a, 2, 3, 32, 4, pos, nullptr, dd, nullptr), "descriptors desc");
  expect_einval(rgan_swd_descriptors(a, 2, 3, 32, 4, pos, b, nullptr, nullptr), "descriptors part");
  expect_einval(rgan_swd_normalize(nullptr, 8, 3, dd, 2, st, nullptr), "normalize desc");
  expect_einval(rgan_swd_normalize(a, 8, 3, nullptr, 2, st, nullptr), "normalize part");
  expect_einval(rgan_swd_normalize(a, 8, 3, dd, 2, nullptr, nullptr), "normalize stats");
  expect_einval(rgan_swd_unit_columns(nullptr, 49, 8, nullptr), "unit_columns dirs");
  expect_einval(rgan_swd_project(nullptr, b, 8, 49, 8, c, nullptr), "project desc");
  expect_einval(rgan_swd_project(a, nullptr, 8, 49, 8, c, nullptr), "project dirs");
  expect_einval(rgan_swd_project(a, b, 8, 49, 8, nullptr, nullptr), "project proj");
  expect_einval(rgan_swd_l1(nullptr, b, 8, dd, ws, big, nullptr), "l1 a");
  expect_einval(rgan_swd_l1(a, nullptr, 8, dd, ws, big, nullptr), "l1 b");
  expect_einval(rgan_swd_l1(a, b, 8, nullptr, ws, big, nullptr), "l1 out");
  expect_einval(rgan_swd_l1(a, b, 8, dd, nullptr, big, nullptr), "l1 ws");
  expect_einval(rgan_swd_l1(a, b, 8, dd, ws, 0, nullptr), "l1 short ws");
  expect_einval(rgan_sort_segments(nullptr, b, c, 2, 8, ws, big, nullptr), "sort in");
  expect_einval(rgan_sort_segments(a, nullptr, c, 2, 8, ws, big, nullptr), "sort out");
  expect_einval(rgan_sort_segments(a, b, nullptr, 2, 8, ws, big, nullptr), "sort tmp");
  expect_einval(rgan_sort_segments(a, b, c, 2, 8, nullptr, big, nullptr), "sort ws");
  expect_einval(rgan_sort_segments(a, b, b, 2, 8, ws, big, nullptr), "sort tmp == out");
  expect_einval(rgan_sort_segments(a, b, a, 2, 8, ws, big, nullptr), "sort tmp == in");
  expect_einval(rgan_sort_segments(a, b, c, 2, 8, ws, 0, nullptr), "sort short ws");
  expect(rgan_sort_segments_tile() >= 64, "sort tile");

  // ---- sizes: one bad at a time over the extremes, pointers valid
  for (int v : kInts) {
    if (v <= 0) {
      expect_einval(rgan_swd_load_u8(u8, v, 3, 32, chw, a, nullptr), "load_u8 N");
      expect_einval(rgan_swd_load_u8(u8, 2, v, 32, chw, a, nullptr), "load_u8 C");
      expect_einval(rgan_swd_load_u8(u8, 2, 3, v, chw, a, nullptr), "load_u8 S");
      expect_einval(rgan_swd_pyr_down(a, v, 3, 32, b, nullptr), "pyr_down N");
      expect_einval(rgan_swd_pyr_down(a, 2, v, 32, b, nullptr), "pyr_down C");
      expect_einval(rgan_swd_laplace(a, b, v, 3, 32, c, nullptr), "laplace N");
      expect_einval(rgan_swd_laplace(a, b, 2, v, 32, c, nullptr), "laplace C");
      expect_einval(rgan_swd_positions(a, v, 32, pos, nullptr), "positions n");
      expect_einval(rgan_swd_descriptors(a, v, 3, 32, 4, pos, b, dd, nullptr), "descriptors N");
      expect_einval(rgan_swd_descriptors(a, 2, v, 32, 4, pos, b, dd, nullptr), "descriptors C");
      expect_einval(rgan_swd_descriptors(a, 2, 3, 32, v, pos, b, dd, nullptr), "descriptors P");
      expect_einval(rgan_swd_normalize(a, v, 3, dd, 2, st, nullptr), "normalize M");
      expect_einval(rgan_swd_normalize(a, 8, v, dd, 2, st, nullptr), "normalize C");
      expect_einval(rgan_swd_normalize(a, 8, 3, dd, v, st, nullptr), "normalize nparts");
      expect_einval(rgan_swd_unit_columns(a, v, 8, nullptr), "unit_columns K");
      expect_einval(rgan_swd_unit_columns(a, 49, v, nullptr), "unit_columns D");
      expect_einval(rgan_swd_project(a, b, v, 49, 8, c, nullptr), "project M");
      expect_einval(rgan_swd_project(a, b, 8, v, 8, c, nullptr), "project K");
      expect_einval(rgan_swd_project(a, b, 8, 49, v, c, nullptr), "project D");
      expect_einval(rgan_swd_l1(a, b, v, dd, ws, big, nullptr), "l1 n");
      expect_einval(rgan_sort_segments(a, b, c, v, 8, ws, big, nullptr), "sort nseg");
      expect_einval(rgan_sort_segments(a, b, c, 2, v, ws, big, nullptr), "sort len");
    }
    if (v > 4) {
      expect_einval(rgan_swd_load_u8(u8, 2, v, 32, chw, a, nullptr), "load_u8 C > 4");
      expect_einval(rgan_swd_descriptors(a, 2, v, 32, 4, pos, b, dd, nullptr), "descriptors C > 4");
      expect_einval(rgan_swd_normalize(a, 8, v, dd, 2, st, nullptr), "normalize C > 4");
    }
    if (v < 32 || !pow2(v)) {
      expect_einval(rgan_swd_pyr_down(a, 2, 3, v, b, nullptr), "pyr_down S");
      expect_einval(rgan_swd_laplace(a, b, 2, 3, v, c, nullptr), "laplace S");
    }
    if (v < 7) {
      expect_einval(rgan_swd_positions(a, 8, v, pos, nullptr), "positions side");
      expect_einval(rgan_swd_descriptors(a, 2, 3, v, 4, pos, b, dd, nullptr), "descriptors side");
    }
    if (v > 196) expect_einval(rgan_swd_unit_columns(a, v, 8, nullptr), "unit_columns K > 196");
    if (v > 196) expect_einval(rgan_swd_project(a, b, 8, v, 8, c, nullptr), "project K > 196");
    if (v > 512) expect_einval(rgan_swd_unit_columns(a, 49, v, nullptr), "unit_columns D > 512");
    if (v > 512) expect_einval(rgan_swd_project(a, b, 8, 49, v, c, nullptr), "project D > 512");
  }
  // products past the limits
  expect_einval(rgan_sort_segments(a, b, c, 1 << 16, 1 << 15, ws, big, nullptr), "sort nseg len == 2^31");
  expect_einval(rgan_sort_segments(a, b, c, 2147483647, 2147483647, ws, big, nullptr), "sort nseg len huge");
  expect_einval(rgan_sort_segments(a, b, c, 2, 1 << 30, ws, big, nullptr), "sort 2 x 2^30");
  expect_einval(rgan_swd_project(a, b, 1 << 23, 49, 256, c, nullptr), "project M D == 2^31");
  expect_einval(rgan_swd_descriptors(a, 1 << 20, 3, 32, 1 << 11, pos, b, dd, nullptr), "descriptors N P == 2^31");
  expect_einval(rgan_swd_load_u8(u8, 2147483647, 4, 2147483647, chw, a, nullptr), "load_u8 huge");
  expect_einval(rgan_swd_pyr_down(a, 2147483647, 4, 1 << 30, b, nullptr), "pyr_down huge");
  expect_einval(rgan_swd_laplace(a, b, 2147483647, 4, 1 << 30, c, nullptr), "laplace huge");
  expect_einval(rgan_swd_l1(a, b, 1ll << 31, dd, ws, big, nullptr), "l1 n == 2^31");
  expect_einval(rgan_swd_l1(a, b, 9223372036854775807ll, dd, ws, big, nullptr), "l1 n huge");
  expect_einval(rgan_swd_normalize(a, 1ll << 31, 3, dd, 2, st, nullptr), "normalize M == 2^31");
  expect_einval(rgan_swd_normalize(a, 9223372036854775807ll, 3, dd, 2, st, nullptr), "normalize M huge");
  expect_einval(rgan_swd_positions(a, 9223372036854775807ll, 32, pos, nullptr), "positions n huge");

  // ---- the workspace sizes at every pair of extremes: no overflow, 0 for what the call refuses
  for (int x : kInts)
    for (int y : kInts) {
      const size_t s = rgan_sort_segments_ws_bytes(x, y);
      const bool ok = x > 0 && y > 0 && (long long)x * y < (1ll << 31);
      expect(ok ? (s >= 1024 && s <= (size_t)1 << 42) : s == 0, "sort ws_bytes");
      const size_t t = rgan_swd_stats_ws_bytes(x, y);
      expect((x > 0 && y > 0 && y <= 4) ? (t == ((size_t)x * y + y) * 16) : t == 0, "stats ws_bytes");
    }
  for (long long n : {-9223372036854775807ll - 1, -1ll, 0ll, 1ll, 255ll, 256ll, 257ll, 262144ll, (1ll << 31) - 1, 1ll << 31,
                      9223372036854775807ll}) {
    const size_t s = rgan_swd_l1_ws_bytes(n);
    expect((n > 0 && n < (1ll << 31)) ? (s >= 8 && s <= 8192) : s == 0, "l1 ws_bytes");
  }

  if (g_fail) {
    std::fprintf(stderr, "%d of %lld calls failed\n", g_fail, g_calls);
    return 1;
  }
  std::printf("swd_args ok: %lld calls\n", g_calls);
  return 0;
}
