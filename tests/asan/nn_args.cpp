// Host-side argument checks of the rgan_nn_ entry points under AddressSanitizer + UBSan, CPU only
// (a stand-alone companion of abi_fuzz.cpp, lecam_args.cpp and swd_args.cpp).
//
// Built by tests/test_nn_cpu.py from csrc/nn.hip with -fsanitize=address,undefined on the host half
// only (hipcc -Xarch_host; the device half is compiled normally and never launched).  Every call here
// is malformed in at least one argument and must answer RGAN_EINVAL before any launch (a launch
// attempt on this GPU-less host would return a HIP error instead, reported as a failure); the sizes
// sweep the integer extremes, and the size functions are called over all of them (a signed overflow
// there is a UBSan report).
//
// Exit 0 and one "nn_args ok" line, or a sanitizer report / a list of failures.
#include <climits>
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

static const std::vector<int> kInts = {INT_MIN, -65536, -64, -7, -1, 0, 1, 2, 3, 7, 8, 9, 16, 31, 32, 33, 63, 64,
                                       65, 96, 127, 128, 129, 192, 255, 256, 4096, 4097, 12288, 12289, 12352, 65536,
                                       1 << 20, 1 << 28, INT_MAX};
static const std::vector<long long> kOffsets = {LLONG_MIN, LLONG_MIN + 1, -(1ll << 40), -1, 0, 1, 37, 1ll << 40,
                                                LLONG_MAX - 1, LLONG_MAX};

static bool side_ok(int s) { return s == 8 || s == 16 || s == 32 || s == 64; }
static bool row_ok(int rb) { return rb >= 64 && rb % 64 == 0 && rb <= RGAN_NN_MAX_ROW_BYTES; }

int main() {
  // dummies: never dereferenced on the host, and no call below may reach the device
  const uint8_t* u8 = reinterpret_cast<const uint8_t*>(0x1000);
  const int8_t* a = reinterpret_cast<const int8_t*>(0x2000);
  const int8_t* b = reinterpret_cast<const int8_t*>(0x3000);
  const int8_t* odd = reinterpret_cast<const int8_t*>(0x3008);
  int8_t* desc = reinterpret_cast<int8_t*>(0x4000);
  int* na = reinterpret_cast<int*>(0x5000);
  int* nb = reinterpret_cast<int*>(0x6000);
  int* dist = reinterpret_cast<int*>(0x7000);
  int* idx = reinterpret_cast<int*>(0x8000);
  void* ws = reinterpret_cast<void*>(0x9000);
  void* ws4 = reinterpret_cast<void*>(0x9004);
  const long long chw[4] = {3 * 32 * 32, 32 * 32, 32, 1};
  const long long bad[4] = {3 * 32 * 32, 32 * 32, -32, 1};
  const long long huge[4] = {LLONG_MAX, 32 * 32, 32, 1};
  const size_t big = ~(size_t)0;

  // ---- null pointers and bad pointers, sizes valid
  expect_einval(rgan_nn_pack_u8(nullptr, 2, 3, 32, chw, 16, desc, na, nullptr), "pack in");
  expect_einval(rgan_nn_pack_u8(u8, 2, 3, 32, nullptr, 16, desc, na, nullptr), "pack strides");
  expect_einval(rgan_nn_pack_u8(u8, 2, 3, 32, chw, 16, nullptr, na, nullptr), "pack desc");
  expect_einval(rgan_nn_pack_u8(u8, 2, 3, 32, chw, 16, desc, nullptr, nullptr), "pack norm");
  expect_einval(rgan_nn_pack_u8(u8, 2, 3, 32, bad, 16, desc, na, nullptr), "pack negative stride");
  expect_einval(rgan_nn_pack_u8(u8, 2, 3, 32, huge, 16, desc, na, nullptr), "pack huge stride");
  expect_einval(rgan_nn_topk(nullptr, na, 5, b, nb, 7, 64, 3, 0, 1, dist, idx, ws, big, nullptr), "topk a");
  expect_einval(rgan_nn_topk(a, nullptr, 5, b, nb, 7, 64, 3, 0, 1, dist, idx, ws, big, nullptr), "topk na");
  expect_einval(rgan_nn_topk(a, na, 5, nullptr, nb, 7, 64, 3, 0, 1, dist, idx, ws, big, nullptr), "topk b");
  expect_einval(rgan_nn_topk(a, na, 5, b, nullptr, 7, 64, 3, 0, 1, dist, idx, ws, big, nullptr), "topk nb");
  expect_einval(rgan_nn_topk(a, na, 5, b, nb, 7, 64, 3, 0, 1, nullptr, idx, ws, big, nullptr), "topk dist");
  expect_einval(rgan_nn_topk(a, na, 5, b, nb, 7, 64, 3, 0, 1, dist, nullptr, ws, big, nullptr), "topk idx");
  expect_einval(rgan_nn_topk(a, na, 5, b, nb, 7, 64, 3, 0, 1, dist, idx, nullptr, big, nullptr), "topk ws");
  expect_einval(rgan_nn_topk(odd, na, 5, b, nb, 7, 64, 3, 0, 1, dist, idx, ws, big, nullptr), "topk a alignment");
  expect_einval(rgan_nn_topk(a, na, 5, odd, nb, 7, 64, 3, 0, 1, dist, idx, ws, big, nullptr), "topk b alignment");
  expect_einval(rgan_nn_topk(a, na, 5, b, nb, 7, 64, 3, 0, 1, dist, idx, ws4, big, nullptr), "topk ws alignment");
  expect_einval(rgan_nn_topk(a, na, 5, b, nb, 7, 64, 3, 0, 1, dist, idx, ws, 5 * 3 * 8 - 1, nullptr), "topk short ws");
  expect_einval(rgan_nn_topk(a, na, 5, b, nb, 7, 64, 3, 0, 0, dist, idx, ws, 0, nullptr), "topk no ws");
  expect_einval(rgan_nn_covered(nullptr, na, 5, b, nb, dist, 7, 64, 0, idx, nullptr), "covered a");
  expect_einval(rgan_nn_covered(a, nullptr, 5, b, nb, dist, 7, 64, 0, idx, nullptr), "covered na");
  expect_einval(rgan_nn_covered(a, na, 5, nullptr, nb, dist, 7, 64, 0, idx, nullptr), "covered b");
  expect_einval(rgan_nn_covered(a, na, 5, b, nullptr, dist, 7, 64, 0, idx, nullptr), "covered nb");
  expect_einval(rgan_nn_covered(a, na, 5, b, nb, nullptr, 7, 64, 0, idx, nullptr), "covered radius");
  expect_einval(rgan_nn_covered(a, na, 5, b, nb, dist, 7, 64, 0, nullptr, nullptr), "covered flag");
  expect_einval(rgan_nn_covered(odd, na, 5, b, nb, dist, 7, 64, 0, idx, nullptr), "covered a alignment");
  expect_einval(rgan_nn_covered(a, na, 5, odd, nb, dist, 7, 64, 0, idx, nullptr), "covered b alignment");

  // ---- the size functions over every pair of extremes, and pack over (C, S, s)
  for (int C : kInts)
    for (int s : kInts) {
      const size_t rb = rgan_nn_row_bytes(C, s);
      const bool legal = C >= 1 && C <= 4 && side_ok(s) && (size_t)C * s * s <= RGAN_NN_MAX_ROW_BYTES;
      expect(legal ? (rb >= (size_t)C * s * s && rb % 64 == 0 && rb < (size_t)C * s * s + 64) : rb == 0, "row_bytes");
      for (int S : kInts) {
        const bool ok = legal && S >= 1 && S % s == 0 && S / s <= 32;
        if (!ok) expect_einval(rgan_nn_pack_u8(u8, 2, C, S, chw, s, desc, na, nullptr), "pack sizes");
      }
    }
  for (int N : {INT_MIN, -1, 0}) expect_einval(rgan_nn_pack_u8(u8, N, 3, 32, chw, 16, desc, na, nullptr), "pack N");

  for (int Q : kInts)
    for (int R : kInts) {
      const int ns = rgan_nn_topk_splits(Q, R);
      expect((Q >= 1 && R >= 1) ? (ns >= 1 && ns <= 4096) : ns == 0, "topk_splits");
      for (int k : {INT_MIN, -1, 0, 1, 3, 8, 9, INT_MAX})
        for (int nsplit : {INT_MIN, -1, 0, 1, 7, 4096, 4097, INT_MAX}) {
          const size_t bytes = rgan_nn_topk_ws_bytes(Q, R, k, nsplit);
          const bool sizes = Q >= 1 && R >= 1 && k >= 1 && k <= 8 && nsplit >= 0 && nsplit <= 4096;
          const long long n = sizes ? (long long)Q * (nsplit ? nsplit : ns) * k : 0;
          const bool legal = sizes && n <= INT_MAX;
          expect(legal ? bytes == (size_t)n * 8 : bytes == 0, "topk_ws_bytes");
          if (!legal)
            for (long long off : kOffsets)
              expect_einval(rgan_nn_topk(a, na, Q, b, nb, R, 64, k, off, nsplit, dist, idx, ws, big, nullptr),
                            "topk sizes");
        }
      if (Q < 1 || R < 1)
        for (long long off : kOffsets)
          expect_einval(rgan_nn_covered(a, na, Q, b, nb, dist, R, 64, off, idx, nullptr), "covered sizes");
    }
  for (int rb : kInts)
    if (!row_ok(rb)) {
      expect_einval(rgan_nn_topk(a, na, 5, b, nb, 7, rb, 3, 0, 1, dist, idx, ws, big, nullptr), "topk row_bytes");
      expect_einval(rgan_nn_covered(a, na, 5, b, nb, dist, 7, rb, 0, idx, nullptr), "covered row_bytes");
    }

  if (g_fail) {
    std::fprintf(stderr, "%d of %lld checks failed\n", g_fail, g_calls);
    return 1;
  }
  std::printf("nn_args ok (%lld checks)\n", g_calls);
  return 0;
}
