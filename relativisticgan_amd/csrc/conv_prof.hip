// The launch profiler of the convolution path and its rgan_profile_* entry points.
#include "conv_plan.h"

#include <cstdarg>
#include <string>
#include <vector>

namespace rgan {

// When enabled (rgan_profile_begin), every GEMM launch is bracketed by a pair of HIP
// events on its own stream and tagged with the algorithmic FLOPs of the conv op it
// serves (2*B*Cin*Cout*k*k*pixels, the torch flop-counter convention) and with the
// kernel instantiation, so bench.py can report FLOPs / kernel time per kernel symbol.
// The name comes from the function that launches the kernel (prof_kernel, called inside
// timed_launch's bracket): there is no table of kernels, only the names seen so far.
struct ProfRec {
  hipEvent_t a, b;
  double flops;
  int kernel;  // index into g_names, -1 until named
};
static bool g_prof = false;
static std::vector<hipEvent_t> g_pool;
static std::vector<ProfRec> g_recs;
static std::vector<std::string> g_names;  // every kernel name recorded so far, in order of first launch
static double g_cur_flops = 0.0;
static ProfRec g_open{};
static bool g_is_open = false;

void prof_kernel(const char* fmt, ...) {
  if (!g_is_open) return;
  char buf[160];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  size_t i = 0;
  while (i < g_names.size() && g_names[i] != buf) ++i;
  if (i == g_names.size()) g_names.emplace_back(buf);
  g_open.kernel = (int)i;
}

void prof_set_flops(double flops) { g_cur_flops = flops; }

// One launch (a kernel and what follows it on the narrow paths) between two events: timed_launch
// (conv_plan.h) calls prof_open, the launch, then prof_close with the launch's status.
void prof_open(hipStream_t s) {
  g_is_open = g_prof && g_recs.size() * 2 + 2 <= g_pool.size();
  if (g_is_open) {
    g_open.a = g_pool[g_recs.size() * 2];
    g_open.b = g_pool[g_recs.size() * 2 + 1];
    g_open.flops = g_cur_flops;
    g_open.kernel = -1;
    hipEventRecord(g_open.a, s);
  }
}

int prof_close(hipStream_t s, int rc) {
  if (!rc) rc = (int)hipGetLastError();
  if (!rc && g_is_open) {
    hipEventRecord(g_open.b, s);
    g_recs.push_back(g_open);
  }
  g_is_open = false;  // on every path: prof_kernel outside a bracket does nothing
  return rc;
}

}  // namespace rgan

using namespace rgan;

extern "C" int rgan_profile_begin(int capacity) {
  if (capacity <= 0) return RGAN_EINVAL;
  for (auto e : g_pool) hipEventDestroy(e);
  g_pool.clear();
  g_recs.clear();
  g_pool.resize((size_t)capacity * 2);
  for (auto& e : g_pool) {
    hipError_t rc = hipEventCreate(&e);
    if (rc != hipSuccess) return (int)rc;
  }
  g_prof = true;
  return 0;
}

// Stops recording, waits for the last event and returns totals over all recorded GEMM
// launches; per-kernel-symbol totals are then available via rgan_profile_kernel.
static std::vector<double> g_kms, g_kflops;
static std::vector<long long> g_kn;

extern "C" int rgan_profile_end(double* total_ms, double* total_flops, long long* launches) {
  g_prof = false;
  g_kms.assign(g_names.size(), 0.0);
  g_kflops.assign(g_names.size(), 0.0);
  g_kn.assign(g_names.size(), 0);
  double ms = 0.0, fl = 0.0;
  if (!g_recs.empty()) {
    hipError_t rc = hipEventSynchronize(g_recs.back().b);
    if (rc != hipSuccess) return (int)rc;
  }
  for (const ProfRec& r : g_recs) {
    float t = 0.f;
    hipError_t rc = hipEventElapsedTime(&t, r.a, r.b);
    if (rc != hipSuccess) return (int)rc;
    ms += t;
    fl += r.flops;
    if (r.kernel < 0) continue;
    g_kms[r.kernel] += t;
    g_kflops[r.kernel] += r.flops;
    g_kn[r.kernel] += 1;
  }
  if (total_ms) *total_ms = ms;
  if (total_flops) *total_flops = fl;
  if (launches) *launches = (long long)g_recs.size();
  g_recs.clear();
  return 0;
}

extern "C" int rgan_profile_kernel(int idx, char* name, int name_len, double* ms, double* flops, long long* n) {
  if (idx < 0 || (size_t)idx >= g_kms.size()) return RGAN_EINVAL;
  if (name && name_len > 0) snprintf(name, name_len, "%s", g_names[idx].c_str());
  if (ms) *ms = g_kms[idx];
  if (flops) *flops = g_kflops[idx];
  if (n) *n = g_kn[idx];
  return 0;
}
