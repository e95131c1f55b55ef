// Host-side argument checks of rgan_diffaug_p, rgan_ada_update and rgan_ada_adjust under
// AddressSanitizer + UBSan, CPU only (a stand-alone companion of abi_fuzz.cpp).
//
// Built by tests/test_ada_cpu.py from csrc/augment.hip and csrc/ada.hip with -fsanitize=address,
// undefined on the host half only (hipcc -Xarch_host; the device half is compiled normally and
// never launched).  Every call here is malformed in at least one argument and must answer
// RGAN_EINVAL before any launch (a launch attempt on this GPU-less host would return a HIP error
// instead, reported as a failure); the integer arguments sweep the extremes, so the size checks
// (batch <= 65535, channels * h * w < 2^31) run on overflowing products under UBSan.
//
// Exit 0 and one "ada_args ok" line, or a sanitizer report / a list of failures.
#include <cstdint>
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

static const std::vector<int> kInts = {-2147483647 - 1, -65536, -7, -1, 0, 1, 2, 3, 4, 5, 7, 8, 16, 31, 32, 33,
                                       64, 128, 129, 1024, 4096, 65535, 65536, 1 << 20, 1 << 28, 2147483647};

int main() {
  // dummies: never dereferenced on the host, and no call below may reach the device
  const float* x = reinterpret_cast<const float*>(0x1000);
  const float* u = reinterpret_cast<const float*>(0x2000);
  const float* gate = reinterpret_cast<const float*>(0x3000);
  const double* p = reinterpret_cast<const double*>(0x4000);
  float* ws = reinterpret_cast<float*>(0x5000);
  float* y = reinterpret_cast<float*>(0x6000);
  double* state = reinterpret_cast<double*>(0x7000);

  // one null pointer at a time, every integer combination of the extremes alongside
  for (int b : kInts)
    for (int c : kInts)
      for (int h : kInts)
        for (int w : {-1, 0, 1, 3, 4, 65536, 2147483647})
          for (int adjoint = 0; adjoint < 2; ++adjoint) {
            expect_einval(rgan_diffaug_p(x, u, nullptr, p, b, c, h, w, 7, adjoint, ws, y, nullptr), "diffaug_p gate");
            expect_einval(rgan_diffaug_p(x, u, gate, nullptr, b, c, h, w, 7, adjoint, ws, y, nullptr), "diffaug_p p");
            expect_einval(rgan_diffaug_p(nullptr, u, gate, p, b, c, h, w, 7, adjoint, ws, y, nullptr), "diffaug_p x");
            expect_einval(rgan_diffaug_p(x, u, gate, p, b, c, h, w, 7, adjoint, ws, const_cast<float*>(x), nullptr),
                          "diffaug_p alias");
            (void)rgan_diffaug_workspace(b, c, h, w);
          }
  // valid pointers, one bad integer
  for (int bad : {-2147483647 - 1, -1, 0}) {
    expect_einval(rgan_diffaug_p(x, u, gate, p, bad, 3, 8, 8, 7, 0, ws, y, nullptr), "diffaug_p batch");
    expect_einval(rgan_diffaug_p(x, u, gate, p, 2, bad, 8, 8, 7, 0, ws, y, nullptr), "diffaug_p channels");
    expect_einval(rgan_diffaug_p(x, u, gate, p, 2, 3, bad, 8, 7, 0, ws, y, nullptr), "diffaug_p h");
    expect_einval(rgan_diffaug_p(x, u, gate, p, 2, 3, 8, bad, 7, 0, ws, y, nullptr), "diffaug_p w");
  }
  for (int policy : {-2147483647 - 1, -1, 8, 64, 2147483647})
    expect_einval(rgan_diffaug_p(x, u, gate, p, 2, 3, 8, 8, policy, 0, ws, y, nullptr), "diffaug_p policy");
  expect_einval(rgan_diffaug_p(x, u, gate, p, 65536, 3, 8, 8, 7, 0, ws, y, nullptr), "diffaug_p batch > 65535");
  expect_einval(rgan_diffaug_p(x, u, gate, p, 2, 2147483647, 2147483647, 2147483647, 7, 0, ws, y, nullptr),
                "diffaug_p sample >= 2^31");
  expect_einval(rgan_diffaug_p(x, u, gate, p, 2, 4, 32768, 32768, 7, 0, ws, y, nullptr), "diffaug_p sample = 2^32");

  for (int n : kInts) {
    expect_einval(rgan_ada_update(nullptr, u, n, p, state, 1, nullptr), "ada_update y_real");
    expect_einval(rgan_ada_update(x, nullptr, n, p, state, 0, nullptr), "ada_update y_fake");
    expect_einval(rgan_ada_update(x, u, n, nullptr, state, 1, nullptr), "ada_update hyper");
    expect_einval(rgan_ada_update(x, u, n, p, nullptr, 0, nullptr), "ada_update state");
    if (n <= 0) expect_einval(rgan_ada_update(x, u, n, p, state, n, nullptr), "ada_update n");
  }
  expect_einval(rgan_ada_adjust(nullptr, state, nullptr), "ada_adjust hyper");
  expect_einval(rgan_ada_adjust(p, nullptr, nullptr), "ada_adjust state");

  if (g_fail) {
    std::fprintf(stderr, "%d of %lld calls failed\n", g_fail, g_calls);
    return 1;
  }
  std::printf("ada_args ok: %lld calls\n", g_calls);
  return 0;
}
