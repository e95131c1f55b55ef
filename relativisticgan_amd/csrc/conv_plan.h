// What the host side of the convolution path shares across its units: the argument blocks of the
// pack / dense / narrow kernels, the Plan the planner (conv_plan.hip) fills and run_plan
// (conv_gemm.hip) executes, the tile constants the planner sizes workspaces with, and the
// declaration, once, of every host function that crosses a unit.  (The implicit-GEMM kernel's
// own types are in conv_types.h.)
#pragma once
#include "conv_types.h"

namespace rgan {

// tile and shape constants of the kernels that the planner's conditions and sizes depend on
constexpr int REDBN_QB = 8;             // splitk_reduce_bn (conv_reduce.hip): channel quads per block
constexpr int NARROW_MAX_SPLITS = 8;    // input-channel splits of convt2_narrow_mfma on small grids
constexpr int NM_TR = 16, NM_TC = 32, NM_CH = 16;  // convt2_narrow_mfma: tile rows / columns, channels per chunk
constexpr int N3_MAXC = 256;            // conv3_narrow_out: most input channels
constexpr int N3_WAVES = 4;             // ... waves per block
constexpr int N3W_PIX = 128;            // wgrad3_narrow: most output pixels per block
constexpr int PK_I = 32, PK_O = 8;      // pack_tiled / pack_tiled16: in x out indices per brick
constexpr int PT_K = 32, PT_N = 128;    // pack_t2d: brick of k x n

// weight packing (conv_pack.hip)
struct PackArgs {
  const float* W;
  float* out;
  int K, N, phases;
  FastDiv fpci, fpkw;      // k -> (kh, kw, ci)
  FastDiv fnco, fnkw;      // n -> (nh, nw, co)
  long long s_in, s_out, s_kh, s_kw;
  int KH, KW, flip, convt2;
};

// one-output dense layer (conv_narrow.hip: dense1_*)
struct DenseArgs {
  const float* x;             // fwd/wgrad: input.  dgrad: unused
  long long xsb, xsc, xsh, xsw;
  const float* w;
  const float* wscale;
  const float* bias;
  float* y;                   // fwd: output [b * ysb].  dgrad/wgrad: dy (read)
  long long ysb;
  float* out;                 // dgrad: dx (strides xs*).  wgrad: dW (torch layout)
  int B, C, HW, E;            // E = C * HW
  FastDiv fc, fw;             // e -> (hw, c); hw -> (h, w)
  int act;
  float alpha;
  int vec;
  int accum;                  // wgrad: add into out
};

// narrow-channel kernels (conv_narrow.hip)
struct NarrowArgs {
  const float* x;
  long long xsb, xsc, xsh, xsw;
  int B, H, W, C;         // input grid
  const float* w;         // NARROW_T: packed [C][4][64] (pack_narrow);  NARROW_IN: torch [Cout][C][KH][KW]
  float* y;
  long long ysb, ysc, ysh, ysw;
  int Ho, Wo, Cout;
  int stride, pad;
  const float* bias;
  const float* wscale;
  int act;
  float alpha;
  int x_bytes, y_bytes;   // conv_img_in: byte extents of x and y (< 2^31, buffer descriptors)
  int splits = 1, cps = 0;  // convt2_narrow_mfma: input-channel splits (cps channels each, a multiple of 16)
  float* slab = nullptr;  // ... their raw sums [split][b][co][oh][ow] when splits > 1 (narrow_split_reduce)
  // conv3_narrow_out: weight element (out n, in c, tap t) at
  // w[n * w_sn + c * w_sc + (w_flip ? taps - 1 - t : t)] (torch Conv2d layout: w_sn = C * taps,
  // w_sc = taps; a data gradient reads the kernel transposed and flipped)
  long long w_sn = 0, w_sc = 0;
  int w_flip = 0;
  // wgrad3_narrow: dy (the layer's output gradient) and its strides; blocks of `rows` output rows
  const float* dy = nullptr;
  long long dsb = 0, dsc = 0, dsh = 0, dsw = 0;
  int chunks = 0, rows = 0;
};

struct Plan {
  int mode = MODE_CONV;
  GemmArgs g{};
  int phases = 1;
  int cfg = CFG_L;
  bool av = false, bv = false, fast = false;
  // packing
  bool pack = false;
  const float* prepacked = nullptr;  // caller-owned packed weights (skip packing)
  PackArgs pk{};
  size_t pack_floats = 0, slab_floats = 0;
  // WGRAD tap-major staging (taps_transpose): C of the GEMM -> workspace, then torch layout
  bool tap_stage = false;
  size_t tap_floats = 0;
  // narrow kernels (MODE_NARROW_T / MODE_NARROW_IN)
  NarrowArgs na{};
  long long pn_s_in = 0, pn_s_out = 0;  // narrow pack strides
  // one-output dense layer (MODE_DENSE1): which = 0 fwd, 1 dgrad, 2 wgrad
  DenseArgs da{};
  int dense_op = 0;
  bool img_in = false;  // MODE_NARROW_IN on the windowed kernel (conv_img_in)
  // BatchNorm moments in the vector epilogue (rgan_conv_fwd_bn): caller's [S][2][C] buffer,
  // equal batch segments whose statistics are kept apart, and whether the launch wrote them
  double* bn_part = nullptr;
  int bn_segs = 1;
  bool bn_fused = false;
  // producer post-op (rgan_conv_post): requested, and whether this plan applies it
  const RganPost* post = nullptr;
  bool post_fused = false;
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline void tile_dims(int cfg, int& bm, int& bn) {
  bm = cfg == CFG_N ? 256 : (cfg == CFG_S ? 64 : 128);
  bn = cfg == CFG_L ? 128 : (cfg == CFG_M || cfg == CFG_S ? 64 : 32);
}

// conv_plan.hip: the planner (host only: no kernel, no launch)
extern const float PLACEHOLDER[4];  // 16-B aligned stand-in for the pointers of a size query
int plan_fwd(const RganConv* d, const float* x, const float* w, const float* wscale, const float* bias, float* y,
             int act, float alpha, Plan& p);
int plan_dgrad(const RganConv* d, const float* dy, const float* w, const float* wscale, float* dx, Plan& p);
int plan_wgrad(const RganConv* d, const float* x, const float* dy, float* dw, Plan& p);
int plan_placeholder(const RganConv* d, int which, const float* w, Plan& p);
size_t plan_ws_bytes(const Plan& p);
OutMap make_out(int gh, int gw, int step, long long sb, long long sh, long long sw, int nkw, int nc, long long th,
                long long tw, long long tc);
bool vec_out(const Plan& p, bool check_ptr);
bool taps4x4_out(const GemmArgs& g);
bool bn_epilogue_ok(const Plan& p);
bool bn_reduce_ok(const Plan& p, bool check_ptr);
long long bn_epilogue_segments(const Plan& p);
bool post_ok(const Plan& p, int mode, int nseg, bool check_ptr);
int pack_kind(const PackArgs& a, int& gx, int& gy);
bool pack_t2d_ok(const PackArgs& a);
size_t wgrad3_lds_bytes(int R, int Wo, int CW, int NC);

// conv_reduce.hip
int launch_splitk_reduce(const Plan& p, hipStream_t s);
void launch_taps_transpose(const float* T, float* O, int M, int Cin, long long osb, int accum, hipStream_t s);

// conv_narrow.hip
int run_narrow(Plan& p, const float* packed, hipStream_t s);
int run_narrow3(Plan& p, hipStream_t s);
int run_dense1(const Plan& p, const float* packed, hipStream_t s);
void launch_pack_narrow(const Plan& p, float* out, hipStream_t s);

// conv_pack.hip
void launch_pack(const PackArgs& a, hipStream_t s);
void launch_pack_plan(Plan& p, float* out, hipStream_t s);

// conv_prof.hip: the launch profiler (prof_kernel is declared in conv_types.h).  prof_open /
// prof_close bracket one launch -- a kernel and what follows it on the narrow paths -- between
// two events; prof_close takes the launch's status, adds the hipGetLastError check and returns
// the result.
void prof_set_flops(double flops);  // the algorithmic FLOPs the brackets opened from now on are tagged with
void prof_open(hipStream_t s);
int prof_close(hipStream_t s, int rc);
template <class Launch>
inline int timed_launch(hipStream_t s, Launch launch) {
  prof_open(s);
  return prof_close(s, launch());
}

}  // namespace rgan
