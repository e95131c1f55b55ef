// The conv planner: a layer descriptor -> a Plan (kernel, tiles, splits, weight layout, workspace), and
// the predicates asked of a Plan.  Host code only; tests/test_conv_plan_cpu.py pins it without a GPU.
#include "conv_plan.h"
#include <atomic>

namespace rgan {

// fewest k steps (of BK) per split (round-4 A/B against 2 / 8 / 16: profiles/round4_split_planner_ab.txt)
constexpr int SPLIT_MINK = 4;

// opt-in fp32-on-bf16x6 GEMMs (rgan_set_gemm_emulation)
static std::atomic<int> g_emu{0};
bool emu_bf16x6() { return g_emu.load(std::memory_order_relaxed) == 1; }

// below SMALL_GEMM_FLOPS, smaller tiles instead of a >= SMALL_SPLITS-way split of 128 x 128
// ones: 64 x 64 for the forward / data gradients (round 5: four times the tiles, a quarter of
// the splits, half the slab bytes per output; C4 3.74 -> 3.53 ms/step, run r5q) and for the
// weight gradients of <= 64 output channels (whose 128-row tiles were half empty: C4 9339 /
// 9357 -> 9427 / 9443 img/s, run r5aa), 128 x 64 for the other weight gradients (C4 3.93 ->
// 3.85 ms/step, run r4v; on 64 x 64 they measured slower, run r5r)
constexpr double SMALL_GEMM_FLOPS = 4e9;
constexpr int SMALL_SPLITS = 4;

static void choose_tiling(Plan& p) {
  GemmArgs& g = p.g;
  p.cfg = g.N <= 32 ? CFG_N : (g.N <= 64 ? CFG_M : CFG_L);
  // small forward / data-gradient GEMMs with N <= 64: 64 x 64 tiles, twice the tiles of
  // 128 x 64 and half its splits (C4 3.535 -> 3.43 ms/step, run r5r; weight gradients stay
  // on 128 x 64: 3.535 -> 3.55 with them moved too)
  if (p.cfg == CFG_M && p.mode != MODE_WGRAD && 2.0 * g.M * g.N * g.K * p.phases < SMALL_GEMM_FLOPS && !emu_bf16x6())
    p.cfg = CFG_S;
  // the weight gradient of a thin input layer (N = taps x <= 3 channels <= 32, M = Cout <= 64:
  // arch 1's Conv3x3 3 -> 64, GLI:260): a 256-row tile would be >= 75 % empty rows (round 6)
  if (p.cfg == CFG_N && p.mode == MODE_WGRAD && g.M <= 64 && !emu_bf16x6()) p.cfg = CFG_S;
  // a thin-M forward with many outputs (arch 1's G input Linear, z -> 4 x 4 x 512 as a 1 x 1 conv
  // over a 1 x 1 map, M = B = 32): 64 x 64 tiles, 128 blocks instead of 64 half-empty 128 x 128
  // ones -- 6.2 us per C4 call vs 15.8 (and vs 13.5 for a VALU kernel with LDS-staged rows;
  // round 6, tools/dense_micro.py)
  if (p.mode == MODE_CONV && g.M <= 64 && g.N >= 4096 && g.K <= 512 && !emu_bf16x6()) p.cfg = CFG_S;
  // ... and its weight gradient (M = 8192 outputs, K = B = 32 pixel rows): 64 x 64 tiles, 256 blocks of
  // one k tile instead of 64 -- 6.4 us per C4 call with the bias vs 19.5 (and vs 12.1 for a VALU
  // kernel with LDS-staged rows, round 6)
  if (p.mode == MODE_WGRAD && g.K <= 64 && g.M >= 4096 && !emu_bf16x6()) p.cfg = CFG_S;
  if (p.cfg == CFG_L) {
    const long long t = (long long)ceil_div(g.M, 128) * ceil_div(g.N, 128) * p.phases;
    const int nk = ceil_div(g.K, BK);
    // small GEMMs (arch 1 at 32x32: 0.1-1.5 GFLOP) that would split K 4+ ways: more tiles,
    // fewer splits and less reduce (128 x 64: C4 4.03 -> 3.92 ms/step, run r4t; 64 x 64 for
    // CONV / CONVT2: 3.74 -> 3.53, run r5q); at C1's 8.6-GFLOP GEMMs the same swap loses
    // (round-4 run r4c)
    const double flops = 2.0 * g.M * g.N * g.K * p.phases;
    // (not under the bf16x6 emulation, whose kernels are 128 x 128)
    if (flops < SMALL_GEMM_FLOPS && t * SMALL_SPLITS <= SPLIT_TARGET && nk >= 4 * SMALL_SPLITS && !emu_bf16x6())
      p.cfg = p.mode == MODE_WGRAD && g.M > 64 ? CFG_M : CFG_S;
  }
  int bm, bn;
  tile_dims(p.cfg, bm, bn);
  const int tiles_m = ceil_div(g.M, bm), tiles_n = ceil_div(g.N, bn);
  g.tiles_n = tiles_n;
  const long long tiles = (long long)tiles_m * tiles_n * p.phases;
  const int nk = ceil_div(g.K, BK);
  int splits = 1;
  // two resident 256-thread blocks per CU on 256 CUs (round-1 sweep of this target: 256 / 384 / 768 /
  // 1024 all lost to 512, profiles/round1_splitk_target_sweep.txt)
  constexpr long long target = SPLIT_TARGET;
  if (tiles < target) {
    splits = (int)((target + tiles - 1) / tiles);
    splits = std::min(splits, std::max(1, nk / SPLIT_MINK));
    splits = std::min(splits, 256);
    // bound the slab to 256 MiB
    while (splits > 1 && (size_t)splits * g.M * g.N * p.phases > (size_t)64 << 20) --splits;
  }
  const int per = ceil_div(nk, splits);
  g.ksplit = per * BK;
  g.splits = ceil_div(g.K, g.ksplit);
  if (g.splits < 1) g.splits = 1;
  // [phase][split][M][N] (splitk_reduce), sized in whole tiles
  p.slab_floats = g.splits > 1 ? (size_t)g.splits * tiles * bm * bn : 0;
}

// rows m -> (b, i, j) over a (gh, gw) grid written at step; columns n -> (nh, nw, c) over (.., nkw, nc)
OutMap make_out(int gh, int gw, int step, long long sb, long long sh, long long sw, int nkw, int nc, long long th,
                long long tw, long long tc) {
  OutMap o;
  o.fgw = FastDiv(gw);
  o.fghw = FastDiv((uint32_t)gh * gw);
  o.step = step;
  o.sb = sb; o.sh = sh; o.sw = sw;
  o.fnc = FastDiv(nc);
  o.fnkw = FastDiv(nkw);
  o.th = th; o.tw = tw; o.tc = tc;
  return o;
}

static Img make_img(const float* p, int H, int W, int C, const long long* s /* b,c,h,w */) {
  Img im;
  im.p = p; im.H = H; im.W = W; im.C = C;
  im.sb = s[0]; im.sc = s[1]; im.sh = s[2]; im.sw = s[3];
  // size-1 spatial dims: only index 0 is ever read, so give them the dense NHWC stride (z as
  // [B][C][1][1] -- G's first layer -- then qualifies for the vector/FAST loaders)
  if (W == 1 && im.sc == 1) im.sw = C;
  if (H == 1 && im.sc == 1) im.sh = (long long)W * im.sw;
  return im;
}

static bool vec_img_ok(const Img& im) {
  return im.sc == 1 && im.C % 4 == 0 && im.sh % 4 == 0 && im.sw % 4 == 0 && im.sb % 4 == 0 &&
         aligned16(im.p);
}

// bytes spanned by an image of `batch` samples (largest element offset + 1)
static long long img_span_bytes(const Img& im, int batch) {
  return 4LL * ((long long)(batch - 1) * im.sb + (long long)(im.H - 1) * im.sh + (long long)(im.W - 1) * im.sw +
                (long long)(im.C - 1) * im.sc + 1);
}

// FAST-path eligibility (see gemm_kernel): call after choose_tiling
static void set_fast(Plan& p, int batch) {
  GemmArgs& g = p.g;
  p.fast = false;
  g.im_buf = 0;
  if (p.mode == MODE_WGRAD && !p.bv) {  // the scalar im2col gathers through a descriptor (element offsets < 2^29)
    const long long im_bytes = img_span_bytes(g.im, batch);
    if (im_bytes <= FAST_MAX_BYTES / 4 && g.im.sb >= 0 && g.im.sh >= 0 && g.im.sw >= 0 && g.im.sc >= 0) {
      g.im_bytes = (int)im_bytes;
      g.im_buf = 1;
    }
  }
  if (!p.av || !p.bv || g.K % BK != 0) return;
  int bm, bn;
  tile_dims(p.cfg, bm, bn);
  const long long a_bytes = img_span_bytes(g.a, batch);
  if (a_bytes > FAST_MAX_BYTES) return;
  if (p.mode != MODE_WGRAD) {
    const long long bw = 4LL * g.K * g.N * p.phases;
    if ((int)g.fC.d % BK != 0 || bw > FAST_MAX_BYTES) return;
    g.a_bytes = (int)a_bytes;
    g.bw_bytes = (int)(4LL * g.K * g.N);
  } else {
    const long long im_bytes = img_span_bytes(g.im, batch);
    if (im_bytes > FAST_MAX_BYTES) return;
    if (g.a.sh != (long long)g.a.W * g.a.sw || g.a.sb != (long long)g.a.H * g.a.sh) return;
    // a B tile is one tap's BN channels, or BN / Cin <= 4 whole taps of one kernel row
    const int cin = g.im.C;
    if (cin % bn != 0 && !(bn % cin == 0 && cin % 4 == 0 && bn / cin <= 4 && g.KW % (bn / cin) == 0))
      return;
    g.a_bytes = (int)a_bytes;
    g.im_bytes = (int)im_bytes;
  }
  p.fast = true;
}

static void set_pack(Plan& p, const float* W, const float* scale, int K, int N, int pci, int pkw,
                     int nco, int nkw, long long s_in, long long s_out, long long s_kh, long long s_kw,
                     int KH, int KW, int flip, int convt2) {
  p.pack = true;
  p.g.wscale = scale;
  PackArgs& a = p.pk;
  a.W = W; a.K = K; a.N = N; a.phases = p.phases;
  a.fpci = FastDiv(pci); a.fpkw = FastDiv(pkw);
  a.fnco = FastDiv(nco); a.fnkw = FastDiv(nkw);
  a.s_in = s_in; a.s_out = s_out; a.s_kh = s_kh; a.s_kw = s_kw;
  a.KH = KH; a.KW = KW; a.flip = flip; a.convt2 = convt2;
  p.pack_floats = (size_t)K * N * p.phases;
}

static bool desc_ok(const RganConv* d) {
  if (!d) return false;
  if (d->batch <= 0 || d->cin <= 0 || d->cout <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride <= 0 ||
      d->pad < 0 || d->hin <= 0 || d->win <= 0 || d->hout <= 0 || d->wout <= 0 ||
      (d->transposed != 0 && d->transposed != 1))
    return false;
  // sizes bounded before any arithmetic on them (every product below stays in 64 bits)
  constexpr int DMAX = 1 << 24, KMAX = 256;
  if (d->batch > DMAX || d->cin > DMAX || d->cout > DMAX || d->hin > DMAX || d->win > DMAX || d->hout > DMAX ||
      d->wout > DMAX || d->kh > KMAX || d->kw > KMAX || d->stride > KMAX || d->pad > KMAX)
    return false;
  const long long hin = d->hin, win = d->win, kh = d->kh, kw = d->kw, st = d->stride, pad = d->pad;
  if (!d->transposed) {
    if (hin + 2 * pad < kh || win + 2 * pad < kw) return false;
    if (d->hout != (hin + 2 * pad - kh) / st + 1) return false;
    if (d->wout != (win + 2 * pad - kw) / st + 1) return false;
  } else {
    if (d->hout != (hin - 1) * st - 2 * pad + kh) return false;
    if (d->wout != (win - 1) * st - 2 * pad + kw) return false;
  }
  // 32-bit index space for the GEMM dims
  if ((long long)d->batch * d->hout * d->wout >= (1LL << 31)) return false;
  if ((long long)d->batch * d->hin * d->win >= (1LL << 31)) return false;
  // kernel / channel sizes whose products (K = taps x channels, N = taps x outputs of the 1x1
  // expansion, packed-weight sizes) stay in int; non-negative strides whose extents stay far
  // inside 64-bit offsets (the host-side fuzz of tests/test_host_asan.py)
  const long long taps = kh * kw;
  if (taps * d->cin >= (1LL << 31) || taps * d->cout >= (1LL << 31) || (long long)d->cin * d->cout * taps >= (1LL << 40))
    return false;
  constexpr long long SMAX = 1LL << 40;
  double xext = 0.0, yext = 0.0;
  const int xd[4] = {d->batch, d->cin, d->hin, d->win}, yd[4] = {d->batch, d->cout, d->hout, d->wout};
  for (int i = 0; i < 4; ++i) {
    if (d->xs[i] < 0 || d->xs[i] > SMAX || d->ys[i] < 0 || d->ys[i] > SMAX) return false;
    xext += (double)(xd[i] - 1) * (double)d->xs[i];
    yext += (double)(yd[i] - 1) * (double)d->ys[i];
  }
  return xext < (double)SMAX && yext < (double)SMAX;
}

// k4 s2 p1 with exactly doubled (ConvTranspose2d) / halved (Conv2d) map
static bool k4s2p1_x2(const RganConv* d) {
  if (d->kh != 4 || d->kw != 4 || d->stride != 2 || d->pad != 1) return false;
  return d->transposed ? d->hout == 2 * d->hin && d->wout == 2 * d->win
                       : d->hin == 2 * d->hout && d->win == 2 * d->wout;
}

static bool vec_nhwc(const float* p, const long long* s, int C) {
  return s[1] == 1 && C % 4 == 0 && s[0] % 4 == 0 && s[2] % 4 == 0 && s[3] % 4 == 0 && aligned16(p);
}

// the input block of a narrow kernel: pointer, (b, c, h, w) strides, grid
static void set_narrow_x(NarrowArgs& a, const float* x, const long long* xs, int B, int H, int W, int C) {
  a.x = x; a.xsb = xs[0]; a.xsc = xs[1]; a.xsh = xs[2]; a.xsw = xs[3];
  a.B = B; a.H = H; a.W = W; a.C = C;
}

// ... and its output block: pointer, strides, grid, the conv's stride / pad, the epilogue
static void set_narrow_y(NarrowArgs& a, float* y, const long long* ys, int Ho, int Wo, int Cout, int stride, int pad,
                         const float* bias, const float* wscale, int act, float alpha) {
  a.y = y; a.ysb = ys[0]; a.ysc = ys[1]; a.ysh = ys[2]; a.ysw = ys[3];
  a.Ho = Ho; a.Wo = Wo; a.Cout = Cout; a.stride = stride; a.pad = pad;
  a.bias = bias; a.wscale = wscale; a.act = act; a.alpha = alpha;
}

// k4 s2 p1 ConvTranspose2d over input grid x (channels C, NHWC) with nc <= 4 outputs;
// weight element (in ci, out co, kh, kw) at w[ci * s_in + co * s_out + kh * 4 + kw]
static bool plan_narrow_t(Plan& p, int batch, const float* x, const long long* xs, int H, int W, int C,
                          const float* w, long long s_in, long long s_out, int nc, float* y, const long long* ys,
                          const float* wscale, const float* bias, int act, float alpha) {
  if (nc > 4 || !vec_nhwc(x, xs, C)) return false;
  p.mode = MODE_NARROW_T;
  NarrowArgs& a = p.na;
  set_narrow_x(a, x, xs, batch, H, W, C);
  a.w = w;
  set_narrow_y(a, y, ys, 2 * H, 2 * W, nc, 2, 1, bias, wscale, act, alpha);
  p.pack = true;
  p.pack_floats = (size_t)C * 256;
  p.pn_s_in = s_in; p.pn_s_out = s_out;
  // channel splits when the tiles alone cannot fill the chip (two resident blocks per CU)
  const long long ntiles = (long long)batch * ceil_div(H, NM_TR) * ceil_div(W, NM_TC);
  const int chunks = ceil_div(C, NM_CH);
  int splits = 1;
  if (ntiles < 256)
    splits = (int)std::min<long long>(std::min(chunks, NARROW_MAX_SPLITS),
                                      ceil_div(512, (int)std::max<long long>(ntiles, 1)));
  a.cps = ceil_div(chunks, std::max(splits, 1)) * NM_CH;
  a.splits = ceil_div(C, a.cps);
  a.slab = nullptr;
  p.slab_floats = a.splits > 1 ? (size_t)a.splits * batch * nc * 4 * H * W : 0;
  p.pk.W = w;
  return true;
}

// Conv2d with a 4x4 kernel and <= 4 input channels (any input strides)
static bool plan_narrow_in(Plan& p, const RganConv* d, const float* x, const float* w, const float* wscale,
                           const float* bias, float* y, int act, float alpha) {
  if (d->transposed || d->cin > 4 || d->kh != 4 || d->kw != 4) return false;
  p.mode = MODE_NARROW_IN;
  // the wave-tiled kernel (conv_img_in): k4 s2 p1 halving of an image with <= 3 channels,
  // 128-channel tiles, NHWC output, 32-pixel wave tiles (row segments or two 16-wide rows),
  // 16-B window pieces (input rows contiguous and 16-B aligned)
  const long long xext = 4 * (1 + (d->batch - 1) * d->xs[0] + (d->cin - 1) * d->xs[1] + (d->hin - 1) * d->xs[2] +
                              (d->win - 1) * d->xs[3]);
  const long long yext = 4 * (1 + (d->batch - 1) * d->ys[0] + (d->cout - 1) * d->ys[1] + (d->hout - 1) * d->ys[2] +
                              (d->wout - 1) * d->ys[3]);
  p.img_in = k4s2p1_x2(d) && d->cin <= 3 && (d->cout % 128 == 0 || (d->cin == 3 && d->cout % 32 == 0)) &&
             vec_nhwc(y, d->ys, d->cout) &&
             (d->wout == 16 || d->wout % 32 == 0) && ((long long)d->batch * d->hout * d->wout / 32) < (1LL << 31) &&
             d->xs[3] == 1 && d->xs[0] % 4 == 0 && d->xs[1] % 4 == 0 && d->xs[2] % 4 == 0 && d->xs[0] >= 0 &&
             d->xs[1] >= 0 && d->xs[2] >= 0 && ((uintptr_t)x & 15) == 0 && xext < (1LL << 31) && yext < (1LL << 31);
  NarrowArgs& a = p.na;
  set_narrow_x(a, x, d->xs, d->batch, d->hin, d->win, d->cin);
  a.w = w;
  set_narrow_y(a, y, d->ys, d->hout, d->wout, d->cout, d->stride, d->pad, bias, wscale, act, alpha);
  a.x_bytes = (int)std::min(xext, (1LL << 31) - 1);
  a.y_bytes = (int)std::min(yext, (1LL << 31) - 1);
  p.pack = false;
  return true;
}

// Conv2d 3x3 stride 1 with nc <= 4 outputs over an NHWC input of C channels (C % 16 == 0):
// conv3_narrow_out.  Weight element (out n, in c, tap t) at w[n w_sn + c w_sc + (flip ? 8 - t : t)].
static bool plan_narrow3_out(Plan& p, int batch, const float* x, const long long* xs, int H, int W, int C,
                             const float* w, long long w_sn, long long w_sc, int flip, int nc, float* y,
                             const long long* ys, int Ho, int Wo, int pad, const float* wscale, const float* bias,
                             int act, float alpha) {
  if (nc > 4 || C < 4 || C > N3_MAXC || (C & (C - 1)) || xs[1] != 1 || xs[0] % 4 || xs[2] % 4 || xs[3] % 4 ||
      !aligned16(x))
    return false;
  if (Ho != H + 2 * pad - 2 || Wo != W + 2 * pad - 2) return false;
  p.mode = MODE_NARROW3;
  NarrowArgs& a = p.na;
  set_narrow_x(a, x, xs, batch, H, W, C);
  a.w = w; a.w_sn = w_sn; a.w_sc = w_sc; a.w_flip = flip;
  set_narrow_y(a, y, ys, Ho, Wo, nc, 1, pad, bias, wscale, act, alpha);
  // pixels per wave: 64 / (C / 4) per step; enough steps to spread the per-wave weight loads,
  // few enough to leave >= ~8 waves per CU
  const long long P = (long long)batch * Ho * Wo, pw = 64 / (C / 4);
  a.rows = (int)std::max(1LL, std::min(16LL, P / (pw * 2048)));
  // 32-bit pixel indices and a buffer descriptor over x's extent
  const long long ext = ((long long)(batch - 1) * xs[0] + (long long)(H - 1) * xs[2] + (long long)(W - 1) * xs[3] + C) * 4;
  if (P + 64LL * (a.rows + 2) >= (1LL << 31) || ext >= 0x7ffffff0LL || xs[0] < 0 || xs[2] < 0 || xs[3] < 0) return false;
  a.x_bytes = (int)ext;
  p.pack = false;
  return true;
}

// bytes of wgrad3_narrow's LDS staging for R output rows
size_t wgrad3_lds_bytes(int R, int Wo, int CW, int NC) {
  return (size_t)((R + 2) * (Wo + 2) * CW + R * Wo * NC) * 4;
}

// weight gradient of a 3x3 stride-1 pad-1 Conv2d with <= 4 output channels (wgrad3_narrow + the
// WGRAD split reduce)
static bool plan_wgrad3_narrow(Plan& p, const RganConv* d, const float* x, const float* dy, float* dw) {
  if (d->transposed || d->kh != 3 || d->kw != 3 || d->stride != 1 || d->pad != 1 || d->cout > 4)
    return false;
  const int cw = d->cin;
  if (cw % 4 || 9 * (cw / 4) > 1024) return false;
  // R whole output rows per block, staged in LDS
  const int R = std::max(1, std::min(d->hout, N3W_PIX / std::max(1, d->wout)));
  if (wgrad3_lds_bytes(R, d->wout, cw, d->cout) > 64 * 1024) return false;
  p.mode = MODE_NARROW3W;
  NarrowArgs& a = p.na;
  set_narrow_x(a, x, d->xs, d->batch, d->hin, d->win, d->cin);
  a.dy = dy; a.dsb = d->ys[0]; a.dsc = d->ys[1]; a.dsh = d->ys[2]; a.dsw = d->ys[3];
  a.Ho = d->hout; a.Wo = d->wout; a.Cout = d->cout; a.stride = 1; a.pad = d->pad;
  const long long P = (long long)d->batch * d->hout * d->wout;
  a.rows = R;
  a.chunks = d->batch * ceil_div(d->hout, R);
  p.slab_floats = (size_t)a.chunks * d->cout * 9 * d->cin;
  // the reduce: the WGRAD GEMM's [split][M = cout][N = (kh, kw, ci)] slab into torch layout
  GemmArgs& g = p.g;
  g.M = d->cout; g.N = 9 * d->cin; g.K = (int)P; g.splits = a.chunks;
  g.C = dw; g.bias = nullptr; g.wscale = nullptr; g.act = RGAN_ACT_NONE; g.alpha = 0.f; g.pmode = 0;
  g.out = make_out(1, 1, 1, (long long)d->cin * 9, 0, 0, 3, d->cin, 3, 1, 9);
  p.phases = 1;
  p.pack = false;
  return true;
}

// Conv2d(C, 1, k, 1, 0) over exactly a k x k map (x strides d->xs; y / dy at b * ys[0])
static bool plan_dense1(Plan& p, const RganConv* d, int op, const float* x, const float* w, const float* wscale,
                        const float* bias, float* y, float* out, int act, float alpha) {
  if (d->transposed || d->cout != 1 || d->hout != 1 || d->wout != 1 || d->pad != 0 || d->kh != d->hin ||
      d->kw != d->win)
    return false;
  if ((long long)d->batch * d->cin * d->hin * d->win >= (1LL << 31)) return false;
  p.mode = MODE_DENSE1;
  p.dense_op = op;
  p.pack = false;
  if (op != 2) {
    // filter packed in e order: Wp[(kh,kw,ci)] = W[0][ci][kh][kw] (the conv forward pack)
    const int KK = d->kh * d->kw;
    set_pack(p, w, wscale, KK * d->cin, 1, d->cin, d->kw, 1, 1, KK, (long long)d->cin * KK, d->kw, 1, d->kh,
             d->kw, 0, 0);
  }
  DenseArgs& a = p.da;
  a.x = x; a.xsb = d->xs[0]; a.xsc = d->xs[1]; a.xsh = d->xs[2]; a.xsw = d->xs[3];
  a.w = w; a.wscale = wscale; a.bias = bias; a.y = y; a.ysb = d->ys[0]; a.out = out;
  a.B = d->batch; a.C = d->cin; a.HW = d->hin * d->win; a.E = a.C * a.HW;
  a.fc = FastDiv(d->cin); a.fw = FastDiv(d->win);
  a.act = act; a.alpha = alpha;
  return true;
}

// The shape of a GEMM: mode, phases, M x N x K, the conv geometry, the decompositions of m (WGRAD: p)
// over a (gh, gw) grid and of k (WGRAD: n) into (kh, kw over fkw, channel over C).  Before set_pack.
static void gemm_shape(Plan& p, int mode, int phases, int M, int N, int K, int KH, int KW, int stride, int pad,
                       int gh, int gw, int C, int fkw) {
  GemmArgs& g = p.g;
  p.mode = mode; p.phases = phases;
  g.M = M; g.N = N; g.K = K;
  g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad;
  g.fgw = FastDiv(gw); g.fghw = FastDiv((uint32_t)gh * gw);
  g.fC = FastDiv(C); g.fKW = FastDiv(fkw);
}

// ... and the common tail: the two operands' vector flags, tiles and splits, FAST eligibility
static void gemm_finish(Plan& p, bool av, bool bv, int batch) {
  p.av = av; p.bv = bv;
  choose_tiling(p);
  set_fast(p, batch);
}

// forward GEMM over the conv's input x producing y (conv or transposed conv)
int plan_fwd(const RganConv* d, const float* x, const float* w, const float* wscale, const float* bias, float* y,
             int act, float alpha, Plan& p) {
  if (!desc_ok(d)) return RGAN_EINVAL;
  GemmArgs& g = p.g;
  const int KK = d->kh * d->kw;
  const long long* ys = d->ys;
  if (d->transposed && k4s2p1_x2(d) &&
      plan_narrow_t(p, d->batch, x, d->xs, d->hin, d->win, d->cin, w, (long long)d->cout * 16, 16, d->cout, y, d->ys,
                    wscale, bias, act, alpha))
    return 0;
  if (plan_narrow_in(p, d, x, w, wscale, bias, y, act, alpha)) return 0;
  if (plan_dense1(p, d, 0, x, w, wscale, bias, y, nullptr, act, alpha)) return 0;
  if (!d->transposed && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->cout <= 4 &&
      plan_narrow3_out(p, d->batch, x, d->xs, d->hin, d->win, d->cin, w, (long long)d->cin * 9, 9, 0, d->cout, y,
                       d->ys, d->hout, d->wout, d->pad, wscale, bias, act, alpha))
    return 0;
  g.a = make_img(x, d->hin, d->win, d->cin, d->xs);
  g.C = y; g.bias = bias; g.act = act; g.alpha = alpha;
  if (!d->transposed) {
    gemm_shape(p, MODE_CONV, 1, d->batch * d->hout * d->wout, d->cout, KK * d->cin, d->kh, d->kw, d->stride, d->pad,
               d->hout, d->wout, d->cin, d->kw);
    g.out = make_out(d->hout, d->wout, 1, ys[0], ys[2], ys[3], 1, d->cout, 0, 0, ys[1]);
    // Wp[(kh,kw,ci)][co] = W[co][ci][kh][kw]
    set_pack(p, w, wscale, g.K, g.N, d->cin, d->kw, d->cout, 1, KK, (long long)d->cin * KK, d->kw, 1,
             d->kh, d->kw, 0, 0);
  } else if (k4s2p1_x2(d)) {
    gemm_shape(p, MODE_CONVT2, 4, d->batch * d->hin * d->win, d->cout, 4 * d->cin, 4, 4, 2, 1, d->hin, d->win,
               d->cin, 2);
    g.out = make_out(d->hin, d->win, 2, ys[0], ys[2], ys[3], 1, d->cout, 0, 0, ys[1]);
    // ConvT weight [ci][co][kh][kw]
    set_pack(p, w, wscale, g.K, g.N, d->cin, 2, d->cout, 1, (long long)d->cout * 16, 16, 4, 1, 4, 4, 0, 1);
  } else if (d->hin == 1 && d->win == 1 && d->stride == 1 && d->pad == 0) {
    // 1x1 -> kh x kw expansion (G's first layer, GLI:336): plain GEMM, N = (oh, ow, co).  Every epilogue
    // and reduce reads bias[n], which is the output channel only where n = co: no bias here (the
    // networks' expansions have none; tests/test_conv_edges_gpu.py)
    if (bias) return RGAN_EINVAL;
    gemm_shape(p, MODE_CONV, 1, d->batch, KK * d->cout, d->cin, 1, 1, 1, 0, 1, 1, d->cin, 1);
    g.out = make_out(1, 1, 1, ys[0], 0, 0, d->kw, d->cout, ys[2], ys[3], ys[1]);
    // Wp[ci][(oh,ow,co)] = W[ci][co][oh][ow]
    set_pack(p, w, wscale, g.K, g.N, d->cin, 1, d->cout, d->kw, (long long)d->cout * KK, KK, d->kw, 1,
             d->kh, d->kw, 0, 0);
  } else if (d->stride == 1) {
    // stride-1 transposed conv == conv with the flipped kernel and pad k-1-p
    if (d->kh != d->kw) return RGAN_EINVAL;
    gemm_shape(p, MODE_CONV, 1, d->batch * d->hout * d->wout, d->cout, KK * d->cin, d->kh, d->kw, 1,
               d->kh - 1 - d->pad, d->hout, d->wout, d->cin, d->kw);
    g.out = make_out(d->hout, d->wout, 1, ys[0], ys[2], ys[3], 1, d->cout, 0, 0, ys[1]);
    set_pack(p, w, wscale, g.K, g.N, d->cin, d->kw, d->cout, 1, (long long)d->cout * KK, KK, d->kw, 1,
             d->kh, d->kw, 1, 0);
  } else {
    return RGAN_EINVAL;
  }
  gemm_finish(p, vec_img_ok(g.a), g.N % 4 == 0, d->batch);
  return 0;
}

// data gradient: input dy (cout, hout, wout) -> dx (cin, hin, win)
int plan_dgrad(const RganConv* d, const float* dy, const float* w, const float* wscale, float* dx, Plan& p) {
  if (!desc_ok(d)) return RGAN_EINVAL;
  GemmArgs& g = p.g;
  const int KK = d->kh * d->kw;
  const long long* xs = d->xs;
  // Conv2d k4 s2 p1 dgrad == ConvT of dy with W[co][ci] read as [in=co][out=ci]
  if (!d->transposed && k4s2p1_x2(d) &&
      plan_narrow_t(p, d->batch, dy, d->ys, d->hout, d->wout, d->cout, w, (long long)d->cin * 16, 16, d->cin, dx,
                    d->xs, wscale, nullptr, RGAN_ACT_NONE, 0.f))
    return 0;
  if (plan_dense1(p, d, 1, nullptr, w, wscale, nullptr, const_cast<float*>(dy), dx, RGAN_ACT_NONE, 0.f)) return 0;
  // ConvT k4 s2 p1 with <= 4 outputs (G's image layer): its dgrad is a Conv2d over the
  // image with <= 4 input channels, W[ci][co] read as [out=ci][in=co] -- the narrow-in kernel
  if (d->transposed && k4s2p1_x2(d)) {
    RganConv c = *d;
    c.transposed = 0;
    c.cin = d->cout; c.hin = d->hout; c.win = d->wout;
    c.cout = d->cin; c.hout = d->hin; c.wout = d->win;
    for (int i = 0; i < 4; ++i) { c.xs[i] = d->ys[i]; c.ys[i] = d->xs[i]; }
    if (plan_narrow_in(p, &c, dy, w, wscale, nullptr, dx, RGAN_ACT_NONE, 0.f)) return 0;
  }
  // 3x3 stride-1 Conv2d with <= 4 inputs (arch 1's input layer): its data gradient is the conv
  // of dy with the kernel transposed and flipped (pad 2 - p), <= 4 outputs: the narrow-out
  // kernel, W[co][ci][t] read as [out = ci][in = co][8 - t].  (The mirror case -- <= 4 dy
  // channels into the narrow-in MFMA tile with a 3x3 kernel -- measured no faster than the
  // generic GEMM at C4: 21 vs 19 us per call.)
  if (!d->transposed && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->cin <= 4 &&
      plan_narrow3_out(p, d->batch, dy, d->ys, d->hout, d->wout, d->cout, w, 9, (long long)d->cin * 9, 1, d->cin, dx,
                       d->xs, d->hin, d->win, 2 - d->pad, wscale, nullptr, RGAN_ACT_NONE, 0.f))
    return 0;
  g.a = make_img(dy, d->hout, d->wout, d->cout, d->ys);
  g.C = dx; g.bias = nullptr; g.act = RGAN_ACT_NONE; g.alpha = 0.f;
  g.out = make_out(d->hin, d->win, 1, xs[0], xs[2], xs[3], 1, d->cin, 0, 0, xs[1]);
  if (!d->transposed) {
    if (k4s2p1_x2(d)) {
      gemm_shape(p, MODE_CONVT2, 4, d->batch * d->hout * d->wout, d->cin, 4 * d->cout, 4, 4, 2, 1, d->hout, d->wout,
                 d->cout, 2);
      g.out = make_out(d->hout, d->wout, 2, xs[0], xs[2], xs[3], 1, d->cin, 0, 0, xs[1]);
      // W[co][ci][kh][kw] read as a ConvT weight [in=co][out=ci]
      set_pack(p, w, wscale, g.K, g.N, d->cout, 2, d->cin, 1, (long long)d->cin * 16, 16, 4, 1, 4, 4, 0, 1);
    } else if (d->stride == 1 && d->kh == d->kw) {
      gemm_shape(p, MODE_CONV, 1, d->batch * d->hin * d->win, d->cin, KK * d->cout, d->kh, d->kw, 1,
                 d->kh - 1 - d->pad, d->hin, d->win, d->cout, d->kw);
      // Wp[(kh,kw,co)][ci] = W[co][ci][k-1-kh][k-1-kw]
      set_pack(p, w, wscale, g.K, g.N, d->cout, d->kw, d->cin, 1, (long long)d->cin * KK, KK, d->kw, 1,
               d->kh, d->kw, 1, 0);
    } else {
      return RGAN_EINVAL;
    }
  } else {
    // transposed conv's dgrad is the direct conv (same k, s, p) with W[ci][co] as [out=ci][in=co]
    gemm_shape(p, MODE_CONV, 1, d->batch * d->hin * d->win, d->cin, KK * d->cout, d->kh, d->kw, d->stride, d->pad,
               d->hin, d->win, d->cout, d->kw);
    set_pack(p, w, wscale, g.K, g.N, d->cout, d->kw, d->cin, 1, KK, (long long)d->cout * KK, d->kw, 1,
             d->kh, d->kw, 0, 0);
  }
  gemm_finish(p, vec_img_ok(g.a), g.N % 4 == 0, d->batch);
  return 0;
}

// The output map is the torch layout of a 4x4-tap weight, rows a multiple of 16 B: n = (kh, kw, c),
// out[m][c][kh][kw] (tap staging in plan_wgrad, RED_TAPS in launch_splitk_reduce: each adds its own conditions)
bool taps4x4_out(const GemmArgs& g) {
  const OutMap& o = g.out;
  return o.fnkw.d == 4 && (uint32_t)g.N == 16 * o.fnc.d && o.th == 4 && o.tw == 1 && o.tc == 16 && o.sb % 4 == 0;
}

// weight gradient, written in torch weight layout
int plan_wgrad(const RganConv* d, const float* x, const float* dy, float* dw, Plan& p) {
  if (!desc_ok(d)) return RGAN_EINVAL;
  if (plan_dense1(p, d, 2, x, nullptr, nullptr, nullptr, const_cast<float*>(dy), dw, RGAN_ACT_NONE, 0.f)) return 0;
  if (plan_wgrad3_narrow(p, d, x, dy, dw)) return 0;
  GemmArgs& g = p.g;
  const int KK = d->kh * d->kw;
  g.C = dw; g.bias = nullptr; g.act = RGAN_ACT_NONE; g.alpha = 0.f;
  if (!d->transposed) {
    // C[co][(kh,kw,ci)] = sum_p dy[p][co] * im2col(x)[p][(kh,kw,ci)]
    g.a = make_img(dy, d->hout, d->wout, d->cout, d->ys);
    g.im = make_img(x, d->hin, d->win, d->cin, d->xs);
    gemm_shape(p, MODE_WGRAD, 1, d->cout, KK * d->cin, d->batch * d->hout * d->wout, d->kh, d->kw, d->stride, d->pad,
               d->hout, d->wout, d->cin, d->kw);
    g.out = make_out(1, 1, 1, (long long)d->cin * KK, 0, 0, d->kw, d->cin, d->kw, 1, KK);
  } else {
    // ConvT weight [ci][co][kh][kw]: the adjoint conv maps dy (hout) -> x (hin)
    g.a = make_img(x, d->hin, d->win, d->cin, d->xs);
    g.im = make_img(dy, d->hout, d->wout, d->cout, d->ys);
    gemm_shape(p, MODE_WGRAD, 1, d->cin, KK * d->cout, d->batch * d->hin * d->win, d->kh, d->kw, d->stride, d->pad,
               d->hin, d->win, d->cout, d->kw);
    g.out = make_out(1, 1, 1, (long long)d->cout * KK, 0, 0, d->kw, d->cout, d->kw, 1, KK);
  }
  gemm_finish(p, g.a.sc == 1 && g.M % 4 == 0 && g.a.sh % 4 == 0 && g.a.sw % 4 == 0 && g.a.sb % 4 == 0 &&
                     aligned16(g.a.p),
              vec_img_ok(g.im), d->batch);
  // unsplit FAST wgrads with 4x4 taps: row-contiguous staging + taps_transpose
  if (p.fast && g.splits == 1 && p.cfg == CFG_L && taps4x4_out(g) && g.out.fnc.d % 4 == 0) {
    p.tap_stage = true;
    p.tap_floats = (size_t)g.M * g.N;
  }
  return 0;
}

size_t plan_ws_bytes(const Plan& p) {
  const size_t pack = p.prepacked ? 0 : align_up(p.pack_floats * 4, 256);
  return pack + align_up(p.slab_floats * 4, 256) + align_up(p.tap_floats * 4, 256);
}

// Plan of `which` (0 forward, 2 weight gradient, anything else data gradient) with placeholder
// activation pointers, for the size queries and the packers; w: the weights (nullptr: a placeholder).
alignas(16) extern const float PLACEHOLDER[4] = {0, 0, 0, 0};

int plan_placeholder(const RganConv* d, int which, const float* w, Plan& p) {
  const float* t = PLACEHOLDER;
  if (!w) w = t;
  if (which == 0) return plan_fwd(d, t, w, nullptr, nullptr, (float*)t, 0, 0.f, p);
  if (which == 2) return plan_wgrad(d, t, t, (float*)t, p);
  return plan_dgrad(d, t, w, nullptr, (float*)t, p);
}

// pack kernel of a layout: 0 pack_tiled16, 1 pack_tiled (grid gx x gy), -1 pack_weights
int pack_kind(const PackArgs& a, int& gx, int& gy) {
  // tiled when n is one weight index and the taps are contiguous in W
  if (a.fnco.d == (uint32_t)a.N && a.fnkw.d == 1 && a.s_kw == 1 && a.s_kh == a.KW && a.KH * a.KW <= 16 &&
      (!a.convt2 || (a.KH == 4 && a.KW == 4))) {
    if (a.KH == 4 && a.KW == 4 && a.fpci.d % PK_I == 0 && a.N % PK_O == 0 && a.s_in % 4 == 0 && a.s_out % 4 == 0 &&
        aligned16(a.W) && aligned16(a.out)) {
      gx = (int)a.fpci.d / PK_I;
      gy = a.N / PK_O;
      return 0;
    }
    gx = ceil_div((int)a.fpci.d, PK_I);
    gy = ceil_div(a.N, PK_O);
    return 1;
  }
  return -1;
}

// pack_t2d applies: k = ci alone, n = (tap, co) over a [K][Cout][KH][KW]-contiguous W
bool pack_t2d_ok(const PackArgs& a) {
  const int T = a.KH * a.KW;
  return !a.convt2 && !a.flip && a.phases == 1 && a.fpci.d == (uint32_t)a.K && a.fnco.d * T == (uint32_t)a.N &&
         a.fnkw.d == (uint32_t)a.KW && a.s_kw == 1 && a.s_kh == a.KW && a.s_out == T && a.s_in == a.N &&
         a.K % PT_K == 0 && a.N % PT_N == 0 && aligned16(a.W) && aligned16(a.out);
}

// The output n-quads of a CONV / CONVT2 GEMM are contiguous and 4-float aligned (channel-contiguous
// rows: the vector epilogue, the RED_VEC reduce and splitk_reduce_bn write float4s).  check_ptr:
// also the 16-B alignment of the output pointer (the size queries plan without one).
bool vec_out(const Plan& p, bool check_ptr) {
  const GemmArgs& g = p.g;
  const OutMap& o = g.out;
  auto al4 = [](long long v) { return (v & 3) == 0; };
  return p.mode != MODE_WGRAD && o.tc == 1 && o.fnc.d % 4 == 0 && g.N % 4 == 0 && al4(o.th) && al4(o.tw) &&
         al4(o.sb) && al4(o.sh) && al4(o.sw) && (!check_ptr || aligned16(g.C));
}

// whole 64-row segments, none straddling one of the caller's nseg equal batch segments of the M rows
static bool seg64_ok(int M, int nseg) {
  return nseg >= 1 && M % 64 == 0 && (nseg == 1 || (M % nseg == 0 && (M / nseg) % 64 == 0));
}

// The vector epilogue can emit BatchNorm segment moments: 128x128 FAST tiles written whole
// (no split-K slab, no tap staging), column n = output channel, 64-row segments that never
// straddle a phase or one of the caller's batch segments.  Call after vec_out is set.
bool bn_epilogue_ok(const Plan& p) {
  const GemmArgs& g = p.g;
  if (p.mode != MODE_CONV && p.mode != MODE_CONVT2) return false;
  // the 128 x 128 vector epilogue, or the 64 x 64 tile's scalar epilogue (one segment per tile)
  const bool l_vec = p.fast && p.cfg == CFG_L && g.vec_out;
  const bool s_tile = p.cfg == CFG_S && g.act == RGAN_ACT_NONE;
  if (!(l_vec || s_tile) || g.splits != 1 || p.tap_stage) return false;
  if (g.out.fnc.d != (uint32_t)g.N || !seg64_ok(g.M, p.bn_segs)) return false;
  // moments of batch segments kept apart (segs > 1) also need a one-phase GEMM.  post_ok
  // deliberately has no such condition (post_seg finds a row's batch segment inside its own
  // phase): the two differ on purpose
  return p.bn_segs == 1 || p.phases == 1;
}

// The split-K reduce can emit the same segment moments (splitk_reduce_bn): channel-contiguous
// float4 output rows (the RED_VEC shape), n = channel, 64-row segments as above.
bool bn_reduce_ok(const Plan& p, bool check_ptr) {
  const GemmArgs& g = p.g;
  if (p.mode != MODE_CONV && p.mode != MODE_CONVT2) return false;
  if (g.splits <= 1 || p.tap_stage || g.accum || !vec_out(p, check_ptr) || g.N < 4 * REDBN_QB) return false;
  if (g.out.fnc.d != (uint32_t)g.N || !seg64_ok(g.M, p.bn_segs)) return false;
  return p.bn_segs == 1 || p.phases == 1;  // as bn_epilogue_ok
}

long long bn_epilogue_segments(const Plan& p) { return (long long)p.phases * (p.g.M / 64); }

// producer post-op (GemmArgs::pmode): unsplit FAST 128x128 tiles (gemm_post's vector
// epilogue) or split tiles (mode 1: every reduce shape of CONV / CONVT2; mode 2: the BN
// reduce); mode 2 also needs n = channel and 64-row segments that never straddle a phase or
// a batch segment.  Call after vec_out is set.
bool post_ok(const Plan& p, int mode, int nseg, bool check_ptr) {
  const GemmArgs& g = p.g;
  if (p.mode != MODE_CONV && p.mode != MODE_CONVT2) return false;
  if (p.tap_stage || g.accum || g.bias || g.act != RGAN_ACT_NONE) return false;
  const bool whole = g.splits == 1;  // the epilogue sees whole sums
  if (whole && !(p.fast && p.cfg == CFG_L && g.vec_out)) return false;  // gemm_post's epilogue
  if (mode == 1) return true;
  // (any number of phases with nseg > 1, unlike bn_*_ok)
  if (mode != 2 || g.out.fnc.d != (uint32_t)g.N || !seg64_ok(g.M, nseg)) return false;
  if (whole) return p.fast && p.cfg == CFG_L && g.vec_out;
  return vec_out(p, check_ptr) && g.N >= 4 * REDBN_QB;
}

}  // namespace rgan

using namespace rgan;

extern "C" int rgan_set_gemm_emulation(int on) {
  if (on != 0 && on != 1) return -1;
  const int prev = emu_bf16x6() ? 1 : 0;
  g_emu.store(on, std::memory_order_relaxed);
  return prev;
}
