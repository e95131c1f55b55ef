// Host-side argument checks of rgan_lecam and rgan_lecam_finish under AddressSanitizer + UBSan,
// CPU only (a stand-alone companion of abi_fuzz.cpp and ada_args.cpp).
//
// Built by tests/test_lecam_cpu.py from csrc/lecam.hip with -fsanitize=address,undefined on the
// host half only (hipcc -Xarch_host; the device half is compiled normally and never launched).
// Every call here is malformed in at least one argument and must answer RGAN_EINVAL before any
// launch (a launch attempt on this GPU-less host would return a HIP error instead, reported as a
// failure); the two row counts sweep the integer extremes.
//
// Exit 0 and one "lecam_args ok" line, or a sanitizer report / a list of failures.
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

static const std::vector<int> kInts = {-2147483647 - 1, -65536, -7, -1, 0, 1, 2, 3, 63, 64, 65, 255, 256, 257,
                                       1025, 65535, 65536, 1 << 20, 1 << 28, 2147483647};

int main() {
  // dummies: never dereferenced on the host, and no call below may reach the device
  const float* yr = reinterpret_cast<const float*>(0x1000);
  const float* yf = reinterpret_cast<const float*>(0x2000);
  float* dr = reinterpret_cast<float*>(0x3000);
  float* df = reinterpret_cast<float*>(0x4000);
  const double* hyper = reinterpret_cast<const double*>(0x5000);
  double* state = reinterpret_cast<double*>(0x6000);
  double* out = reinterpret_cast<double*>(0x7000);

  for (int n : kInts)
    for (int ng : kInts)
      for (int mode = 0; mode < 2; ++mode) {
        // one pointer rule broken at a time, whatever the counts
        expect_einval(rgan_lecam(nullptr, nullptr, n, ng, hyper, state, nullptr, nullptr, out, mode, nullptr),
                      "lecam both sides null");
        expect_einval(rgan_lecam(nullptr, nullptr, n, ng, hyper, state, dr, df, out, mode, nullptr),
                      "lecam both sides null, gradients given");
        expect_einval(rgan_lecam(nullptr, yf, n, ng, hyper, state, dr, df, out, mode, nullptr),
                      "lecam dy_real for an absent real side");
        expect_einval(rgan_lecam(yr, nullptr, n, ng, hyper, state, dr, df, out, mode, nullptr),
                      "lecam dy_fake for an absent fake side");
        expect_einval(rgan_lecam(yr, yf, n, ng, nullptr, state, dr, df, out, mode, nullptr), "lecam hyper");
        expect_einval(rgan_lecam(yr, yf, n, ng, hyper, nullptr, dr, df, out, mode, nullptr), "lecam state");
        expect_einval(rgan_lecam(yr, yf, n, ng, hyper, state, dr, df, nullptr, mode, nullptr), "lecam out");
        // valid pointers, bad counts
        if (n <= 0 || ng < n) {
          expect_einval(rgan_lecam(yr, yf, n, ng, hyper, state, dr, df, out, mode, nullptr), "lecam n / n_global");
          expect_einval(rgan_lecam(yr, nullptr, n, ng, hyper, state, nullptr, nullptr, out, mode, nullptr),
                        "lecam n / n_global, real only");
          expect_einval(rgan_lecam(nullptr, yf, n, ng, hyper, state, nullptr, df, out, mode, nullptr),
                        "lecam n / n_global, fake only");
        }
      }
  for (int mode : {-2147483647 - 1, -1, 2, 3, 2147483647})
    expect_einval(rgan_lecam(yr, yf, 8, 8, hyper, state, dr, df, out, mode, nullptr), "lecam mode");

  for (int ng : kInts)
    for (int sides : {-2147483647 - 1, -1, 0, 1, 2, 3, 4, 2147483647}) {
      expect_einval(rgan_lecam_finish(nullptr, ng, sides, hyper, state, out, nullptr), "lecam_finish sums");
      expect_einval(rgan_lecam_finish(out, ng, sides, nullptr, state, out, nullptr), "lecam_finish hyper");
      expect_einval(rgan_lecam_finish(out, ng, sides, hyper, nullptr, out, nullptr), "lecam_finish state");
      expect_einval(rgan_lecam_finish(out, ng, sides, hyper, state, nullptr, nullptr), "lecam_finish loss");
      if (ng <= 0 || sides < 1 || sides > 3)
        expect_einval(rgan_lecam_finish(out, ng, sides, hyper, state, out, nullptr), "lecam_finish n_global / sides");
    }

  if (g_fail) {
    std::fprintf(stderr, "%d of %lld calls failed\n", g_fail, g_calls);
    return 1;
  }
  std::printf("lecam_args ok: %lld calls\n", g_calls);
  return 0;
}
