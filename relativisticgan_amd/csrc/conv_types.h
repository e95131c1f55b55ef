// Types, constants and declarations shared by the implicit-GEMM kernels (gemm_body.h with
// gemm_conv.hip / gemm_convt2.hip / gemm_wgrad.hip) and the units around them, which add their own
// in conv_plan.h.  Host functions that cross into the GEMM units are declared here, once.
#pragma once
#include "common.h"

namespace rgan {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Raw-buffer byte offset past every record of a descriptor (< 2^31 bytes): loads return 0.
constexpr int OOB = (int)0x80000000;
// fast-path tensors must fit a buffer descriptor with this margin
constexpr long long FAST_MAX_BYTES = (1LL << 31) - (1LL << 24);

enum { MODE_CONV = 0, MODE_CONVT2 = 1, MODE_WGRAD = 2, MODE_NARROW_T = 3, MODE_NARROW_IN = 4, MODE_DENSE1 = 5,
       MODE_NARROW3 = 6, MODE_NARROW3W = 7 };
constexpr int BK = 32;
// split-K occupancy target (blocks): two resident 256-thread blocks per CU on 256 CUs
constexpr long long SPLIT_TARGET = 512;

// n / d for 0 <= n < 2^31 via multiply-high (host-computed magic numbers)
struct FastDiv {
  uint32_t d, m, l;
  FastDiv() = default;
  explicit FastDiv(uint32_t div) {
    d = div;
    l = 0;
    while ((1u << l) < d) ++l;
    uint64_t one = 1;
    m = (uint32_t)(((one << 32) * ((one << l) - d)) / d + 1);
  }
  __device__ __forceinline__ uint32_t div(uint32_t n) const {
    uint32_t hi = __umulhi(n, m);
    return (uint32_t)(((uint64_t)hi + n) >> l);
  }
};

struct Img {
  const float* p;
  long long sb, sc, sh, sw;
  int H, W, C;
};

struct OutMap {
  FastDiv fgw, fghw;      // row m -> (b, i, j) over (gh, gw)
  int step;
  long long sb, sh, sw;
  FastDiv fnc, fnkw;      // col n -> (nh, nw, c) over (nkh, nkw, nc)
  long long th, tw, tc;
};

struct GemmArgs {
  int M, N, K;
  int ksplit, splits, tiles_n;
  Img a;                  // CONV/CONVT2: x.  WGRAD: gradient image (channel = m)
  Img im;                 // WGRAD: image expanded by im2col
  int KH, KW, stride, pad;
  FastDiv fgw, fghw;      // decomposition of m (CONV/CONVT2) or p (WGRAD)
  FastDiv fC, fKW;        // k (CONV/CONVT2) or n (WGRAD) -> (kh, kw, ci)
  const float* Bw;        // packed weights [phase][N][K]
  float* C;
  OutMap out;
  const float* bias;
  const float* wscale;    // nullable device scalar multiplying the accumulator (spectral 1/sigma)
  int act;
  float alpha;
  float* slab;
  // FAST paths (raw buffer loads, scalar per-tile offsets): descriptor sizes in bytes
  int a_bytes, im_bytes, bw_bytes;
  int im_buf;             // non-FAST WGRAD: the scalar im2col gathers through the im_bytes descriptor
  int vec_out;            // output n-quads contiguous and 16-B aligned (host-checked)
  int xgroup, nph;        // tile order (0: default; 2: blocks sharing weight columns on one XCD; 3: band order,
                          // each XCD a contiguous eighth of the m tiles); phases
  double* bnp;            // nullable: BatchNorm moments of every 64-row output segment (vector epilogue)
  int accum;              // WGRAD: add into C (gradient accumulation) instead of overwriting it
  // FAST conv WGRAD with a bias (rgan_conv_wgrad dbias): the bias gradient sum_p dy[p][m] is
  // formed from the A tiles the GEMM stages anyway (the n-tile-0 blocks); unsplit: written to
  // dbias (added when db_accum), split: per-split doubles dbp[split][M], summed in split order
  // by the WGRAD reduce
  double* dbp;
  float* dbias;
  int db_accum;
  int db_k0;              // first pixel row summed into dbias (a multiple of BK; rgan_conv_wgrad_rows)
  // Post-op for the layer that PRODUCED this GEMM's output operand (rgan_conv_post: a data
  // gradient, or G's image-layer gradient GEMM), applied where the value is final (unsplit
  // epilogue or split-K reduce); px has C's layout (host-checked):
  //   pmode 1: C = v * act'(px), px = the producer's activation output (its act backward);
  //   pmode 2: C = g = v * act'(px * al + be), px = the producer's BatchNorm input y, al/be
  //            from (mean, invstd) pst[k][2N] of batch segment k and gamma/beta, plus the
  //            BatchNorm backward sums (sum g, sum g (y - mean)) of every 64-row segment into
  //            ppart[seg][2][N] in double (seg as bnp's) -- the bn_bwd_partial pass.
  const float* px;
  const float* pst;
  const float* pgam;
  const float* pbet;
  double* ppart;
  int pmode, pact, pnseg;
  float palpha;
};

enum { CFG_L = 0, CFG_M = 1, CFG_N = 2, CFG_S = 3 };

// one GEMM launch as the planner chose it (conv_plan.h: Plan)
struct GemmLaunch {
  const GemmArgs& g;
  int cfg;  // CFG_*
  bool av, bv, fast;
  dim3 grid;
  hipStream_t s;
};

// conv_plan.hip
bool emu_bf16x6();  // opt-in fp32-on-bf16x6 GEMMs (rgan_set_gemm_emulation)
// the launch profiler (conv_prof.hip): the function that launches a kernel names it (printf-style, the demangled
// symbol that bench.py and profiles/*_pmc_traffic.json key on); does nothing while no launch is
// being recorded
void prof_kernel(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
// gemm_conv.hip / gemm_convt2.hip / gemm_wgrad.hip: launch_mode of one GEMM mode each
void launch_gemm_conv(const GemmLaunch& l);
void launch_gemm_convt2(const GemmLaunch& l);
void launch_gemm_wgrad(const GemmLaunch& l);

}  // namespace rgan
