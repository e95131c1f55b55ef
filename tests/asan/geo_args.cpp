// Host-side argument checks of rgan_diffaug_geo and rgan_diffaug_geo_workspace under
// AddressSanitizer + UBSan, CPU only (a stand-alone companion of ada_args.cpp).
//
// Built by tests/test_diffaug_geo_cpu.py from csrc/augment.hip and csrc/augment_geo.hip with
// -fsanitize=address,undefined on the host half only (hipcc -Xarch_host; the device half is
// compiled normally and never launched).  Every call here is malformed in at least one argument
// and must answer RGAN_EINVAL before any launch (a launch attempt on a GPU-less host would return
// a HIP error instead, reported as a failure); the integer arguments sweep the extremes, so the
// size checks (batch <= 65535, channels * h * w < 2^31) run on overflowing products under UBSan,
// with and without a geometric bit (the latter delegates to rgan_diffaug / rgan_diffaug_p).
//
// Exit 0 and one "geo_args ok" line, or a sanitizer report / a list of failures.
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
  const float* v = reinterpret_cast<const float*>(0x3000);
  const float* gate = reinterpret_cast<const float*>(0x4000);
  const double* p = reinterpret_cast<const double*>(0x5000);
  float* ws = reinterpret_cast<float*>(0x6000);
  float* y = reinterpret_cast<float*>(0x7000);

  // one bad pointer at a time, every integer combination of the extremes alongside
  for (int policy : {7, 8, 56, 63})
    for (int b : kInts)
      for (int c : kInts)
        for (int h : kInts)
          for (int w : {-1, 0, 1, 3, 4, 65536, 2147483647}) {
            const int adjoint = (b ^ c ^ h) & 1;
            expect_einval(rgan_diffaug_geo(x, u, v, nullptr, p, b, c, h, w, policy, adjoint, ws, y, nullptr), "gate");
            expect_einval(rgan_diffaug_geo(x, u, v, gate, nullptr, b, c, h, w, policy, adjoint, ws, y, nullptr), "p");
            expect_einval(rgan_diffaug_geo(nullptr, u, v, gate, p, b, c, h, w, policy, adjoint, ws, y, nullptr), "x");
            expect_einval(rgan_diffaug_geo(x, nullptr, v, nullptr, nullptr, b, c, h, w, policy, adjoint, ws, y, nullptr),
                          "u");
            expect_einval(rgan_diffaug_geo(x, u, v, gate, p, b, c, h, w, policy, adjoint, nullptr, y, nullptr), "ws");
            expect_einval(rgan_diffaug_geo(x, u, v, nullptr, nullptr, b, c, h, w, policy, adjoint, ws,
                                           const_cast<float*>(x), nullptr),
                          "alias");
            if (policy & 56)
              expect_einval(rgan_diffaug_geo(x, u, nullptr, gate, p, b, c, h, w, policy, adjoint, ws, y, nullptr), "v");
            (void)rgan_diffaug_geo_workspace(b, c, h, w);
          }
  // valid pointers, one bad integer
  for (int gated = 0; gated < 2; ++gated) {
    const float* g = gated ? gate : nullptr;
    const double* q = gated ? p : nullptr;
    for (int bad : {-2147483647 - 1, -1, 0}) {
      expect_einval(rgan_diffaug_geo(x, u, v, g, q, bad, 3, 8, 8, 63, 0, ws, y, nullptr), "batch");
      expect_einval(rgan_diffaug_geo(x, u, v, g, q, 2, bad, 8, 8, 63, 0, ws, y, nullptr), "channels");
      expect_einval(rgan_diffaug_geo(x, u, v, g, q, 2, 3, bad, 8, 63, 0, ws, y, nullptr), "h");
      expect_einval(rgan_diffaug_geo(x, u, v, g, q, 2, 3, 8, bad, 63, 0, ws, y, nullptr), "w");
    }
    for (int policy : {-2147483647 - 1, -1, 64, 65, 128, 2147483647})
      expect_einval(rgan_diffaug_geo(x, u, v, g, q, 2, 3, 8, 8, policy, 0, ws, y, nullptr), "policy");
    // quarter turns need a square image, whatever else the policy holds
    for (int policy : {16, 17, 24, 48, 63}) {
      expect_einval(rgan_diffaug_geo(x, u, v, g, q, 2, 3, 8, 12, policy, 0, ws, y, nullptr), "rot90 h != w");
      expect_einval(rgan_diffaug_geo(x, u, v, g, q, 2, 3, 9, 8, policy, 1, ws, y, nullptr), "rot90 h != w");
    }
    expect_einval(rgan_diffaug_geo(x, u, v, g, q, 65536, 3, 8, 8, 63, 0, ws, y, nullptr), "batch > 65535");
    expect_einval(rgan_diffaug_geo(x, u, v, g, q, 2, 2147483647, 2147483647, 2147483647, 63, 0, ws, y, nullptr),
                  "sample >= 2^31");
    expect_einval(rgan_diffaug_geo(x, u, v, g, q, 2, 4, 32768, 32768, 63, 0, ws, y, nullptr), "sample = 2^32");
    expect_einval(rgan_diffaug_geo(x, u, v, g, q, 2, 4, 32768, 32768, 40, 1, ws, y, nullptr), "sample = 2^32");
  }
  if (rgan_diffaug_geo_workspace(2, 3, 8, 8) != rgan_diffaug_workspace(2, 3, 8, 8) ||
      rgan_diffaug_geo_workspace(2, 3, 256, 256) != rgan_diffaug_workspace(2, 3, 256, 256) ||
      rgan_diffaug_geo_workspace(0, 3, 8, 8) != 0) {
    std::fprintf(stderr, "FAIL workspace size\n");
    ++g_fail;
  }

  if (g_fail) {
    std::fprintf(stderr, "%d of %lld calls failed\n", g_fail, g_calls);
    return 1;
  }
  std::printf("geo_args ok: %lld calls\n", g_calls);
  return 0;
}
