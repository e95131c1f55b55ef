// Implicit-GEMM convolutions on fp32 MFMA (v_mfma_f32_32x32x2_f32) for gfx950.
//
// Replaces torch.nn.Conv2d / ConvTranspose2d forward and aten::convolution_backward
// on the reference's hot path (GLI:336,361,387,410,428,448; arch 1 GLI:202-223,260-302).
//
// Three GEMM modes, one kernel template:
//   MODE_CONV   C[m][n] = sum_k im2col(x)[m][k] * Wp[k][n]       (Conv2d fwd, ConvT dgrad,
//               stride-1 ConvT fwd / Conv dgrad with a flipped kernel, 1x1 "GEMM" layers)
//   MODE_CONVT2 the same per output phase (oh%2, ow%2) of a k4 s2 p1 ConvTranspose2d
//               (ConvT fwd, Conv dgrad): 4 sub-pixel GEMMs with K = 4*Cin, no zero taps
//   MODE_WGRAD  C[m][n] = sum_p G[p][m] * im2col(img)[p][n]       (weight gradients)
// Activations are NHWC (torch channels_last) inside the path; any (b,c,h,w) strides are
// accepted (NCHW images at the boundary take the scalar gather).  fp32 in, fp32 MFMA
// accumulate: no reduced precision anywhere.
//
// Tiling: 256 threads = 4 waves; block tile BM x BN x BK(32); each wave owns a
// (BM/WM) x (BN/WN) sub-tile of 32x32 MFMA accumulators.  LDS is double buffered with
// register-staged global loads (next tile's loads in flight while the current tile's
// MFMAs run).  LDS images keep every MFMA operand read a conflict-free ds_read_b32:
// m-major tiles use row stride BK+1, k-major tiles BM+4 / BN+4.  Split-K writes fp32
// slabs reduced in fixed order (deterministic) by splitk_reduce.
//
// This header holds the kernel template and its launcher.  gemm_conv.hip, gemm_convt2.hip and
// gemm_wgrad.hip instantiate one GEMM mode each (three compile jobs instead of one); the split-K
// reduces are in conv_reduce.hip, the planner in conv_plan.hip, run_plan in conv_gemm.hip.
#pragma once
#include "conv_types.h"

namespace rgan {

// per-channel BatchNorm affine of the producer (pmode 2): z = y * al + be
__device__ __forceinline__ void post_consts(const GemmArgs& g, int k, int n, float& al, float& be, float& mu) {
  const int c = min(n, g.N - 1);
  const float* st = g.pst + (size_t)k * 2 * g.N;
  mu = st[c];
  al = (g.pgam ? g.pgam[c] : 1.f) * st[g.N + c];
  be = (g.pbet ? g.pbet[c] : 0.f) - mu * al;
}

// batch segment of output row m (pmode 2, pnseg equal segments of the M rows of every phase)
__device__ __forceinline__ int post_seg(const GemmArgs& g, int m) {
  return g.pnseg > 1 ? m / (g.M / g.pnseg) : 0;
}

__device__ __forceinline__ long long row_offset(const OutMap& o, int m, int phase) {
  uint32_t b = o.fghw.div(m);
  uint32_t rem = m - b * o.fghw.d;
  uint32_t i = o.fgw.div(rem);
  uint32_t j = rem - i * o.fgw.d;
  int ph = phase >> 1, pw = phase & 1;
  return (long long)b * o.sb + (long long)(i * o.step + ph) * o.sh + (long long)(j * o.step + pw) * o.sw;
}

__device__ __forceinline__ long long col_offset(const OutMap& o, int n) {
  uint32_t t = o.fnc.div(n);
  uint32_t c = n - t * o.fnc.d;
  uint32_t nh = o.fnkw.div(t);
  uint32_t nw = t - nh * o.fnkw.d;
  return (long long)nh * o.th + (long long)nw * o.tw + (long long)c * o.tc;
}

// FAST (AV && BV only; host checks the conditions in set_fast): every BK tile of a
// CONV/CONVT2 GEMM lies inside one filter tap (Cin % BK == 0), so per-row input offsets
// change only when the tap does and the per-tile advance (channel chunk, weight row
// block) is a wave-uniform scalar passed as the buffer load's soffset: the main loop
// issues almost no VALU (fp32 MFMA shares the VALU datapath on gfx950 --
// SQ_VALU_MFMA_COEXEC_CYCLES = 0 -- so every address instruction costs MFMA cycles).
// WGRAD: the gradient rows are pixel-contiguous (offset = p * pixel stride: scalar
// advance) and the im2col operand reads one tap per block tile (Cin % BN == 0) through
// a per-tile table of pixel offsets built by one wave into LDS two tiles ahead.
template <int MODE, int BM, int BN, int WM, int WN, bool AV, bool BV, bool FAST, bool EMU, bool POST = false>
__device__ __forceinline__ void gemm_body(const GemmArgs& g) {
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  static_assert(TM >= 1 && TN >= 1 && WM * WN == 4, "tile config");
  constexpr bool AK = (MODE == MODE_WGRAD);          // A staged k-major
  // KROW (every FAST path): both operands staged as k-contiguous rows ([m][k], [n][k]);
  // every lane reads 4 consecutive k of its row with one conflict-free ds_read_b128 that
  // feeds 4 MFMA steps.  The k order inside a BK tile is permuted (MFMA step s of lane
  // half h takes k = 16h + s), the same for A and B, so only the fp32 summation order
  // changes.  CONV/CONVT2: the global rows are k-contiguous too (channels; [N][K] weight
  // pack), stores are ds_write_b128 and the row stride is 36 dwords (9 slots: 16 rows hit
  // 16 slots).  WGRAD (SWZ): k = pixel is the global outer index, so each float4 (4
  // consecutive m or n of one pixel) is stored transposed as 4 ds_write_b32 into rows of
  // 32 dwords whose 16-B quads are XOR-swizzled by (row >> 1) & 7: the reads stay
  // conflict-free (slot = 8 (row & 1) + quad ^ swz) and each store instruction (8 channel
  // quads x 4 pixels per half-wave) is at most 2-way (free for ds_write_b32).
  constexpr bool KROW = FAST;
  constexpr bool SWZ = FAST && MODE == MODE_WGRAD;
  constexpr int KROW_LD = SWZ ? BK : BK + 4;
  constexpr int A_LD = KROW ? KROW_LD : AK ? (BM + 4) : (BK + 1);
  constexpr int A_SZ = KROW ? BM * KROW_LD : AK ? BK * (BM + 4) : BM * (BK + 1);
  constexpr int B_LD = KROW ? KROW_LD : BN + 4;
  constexpr int B_SZ = KROW ? BN * KROW_LD : BK * B_LD;
  constexpr int STAGE = A_SZ + B_SZ;
  // The 256x32 narrow-N tile (CFG_N) is single-buffered (two barriers per k tile): its two
  // stages (83 KB) left one resident block per CU; one stage (41.5 KB) gives three.  The
  // 128x64 tile (CFG_M) likewise (two -> five blocks; C3h32 -1.6 %, C1 / C4 unchanged).  The
  // 128x128 tile keeps two stages (single-buffered it lost 9 %: its vector epilogue needs the
  // LDS, and two blocks per CU already hide the one barrier).  The 64x64 tile (CFG_S: small
  // forward / data-gradient GEMMs, one 32x32 accumulator per wave) keeps two stages (36 KB)
  constexpr bool GEMM_SB = !EMU && ((BM == 256 && BN == 32) || (BM == 128 && BN == 64));
  constexpr int EPI_SZ = KROW ? 4 * (GEMM_SB ? 32 : 64) * 72 : 0;  // vector epilogue staging (4 waves x rows x 72)
  // EMU: one (single-buffered) stage of six bf16 planes (A hi/mid/lo, B hi/mid/lo), rows of
  // 32 bf16 = 16 dwords at a 20-dword stride (16 lanes' ds_read_b128 on 16 distinct quads)
  constexpr int EMU_RS = 20, EMU_PLANE = 128 * EMU_RS;  // dwords
  constexpr int MAIN_SZ = EMU ? 6 * EMU_PLANE : GEMM_SB ? STAGE : 2 * STAGE;
  static_assert(!EMU || (FAST && MODE != MODE_WGRAD && BM == 128 && BN == 128), "bf16x6 path: FAST 128x128 CONV/CONVT2");
  __shared__ __attribute__((aligned(16))) float smem[MAIN_SZ > EPI_SZ ? MAIN_SZ : EPI_SZ];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = (wid / WN) * (BM / WM), wn = (wid % WN) * (BN / WN);
  // Tile order.  Default: x = (m tile, n tile), z = (phase, split).  Blocks are dispatched
  // round-robin over the 8 XCDs, so blocks that read the same operand rows are put 8 dispatch
  // slots apart -- one XCD, one L2 -- instead of on 4-8 different L2s.  (The first such
  // order, xgroup 1 -- the n tiles and phases of one m tile on one XCD -- was superseded by
  // the band order 3 below; tools/patches/xgroup1_row_grouping.diff.)  xgroup 2 (layers whose weights outweigh
  // their input: the deep D convs, G's deep data gradients / ConvTs): the blocks that read
  // the same weight columns (the m tiles and phases of one n tile) share an XCD instead, so
  // the weight is fetched into one L2 rather than into every L2 once per m tile.
  int tm_i, tn_i, phase, split, z;
  if (g.xgroup == 2) {
    const int b = blockIdx.x, r = b >> 3, tiles_m = (g.M + BM - 1) / BM, per = tiles_m * g.nph;
    const int q = r % per;
    tn_i = (r / per) * 8 + (b & 7);
    tm_i = q % tiles_m;
    phase = q / tiles_m;
    split = blockIdx.z;
    z = phase * g.splits + split;
  } else if (g.xgroup == 3) {
    // band order: XCD x (dispatch slot b % 8) takes the x-th eighth of the m tiles, in order,
    // each m tile's n tiles and phases back to back -- the blocks in flight on one XCD cover
    // consecutive output rows, which read overlapping input rows (4 x 4 windows, stride 2)
    const int b = blockIdx.x, r = b >> 3, per = g.tiles_n * g.nph;
    const int q = r % per;
    tm_i = (b & 7) * ((g.M + BM - 1) / BM / 8) + r / per;
    tn_i = q % g.tiles_n;
    phase = q / g.tiles_n;
    split = blockIdx.z;
    z = phase * g.splits + split;
  } else {
    const int tile = blockIdx.x;
    tm_i = tile / g.tiles_n;
    tn_i = tile - tm_i * g.tiles_n;
    z = blockIdx.z;
    phase = z / g.splits;
    split = z - phase * g.splits;
  }
  const int m0 = tm_i * BM, n0 = tn_i * BN;
  const int kbeg = split * g.ksplit;
  const int kend = min(g.K, kbeg + g.ksplit);
  const int nk = (kend - kbeg + BK - 1) / BK;
  const int ph = phase >> 1, pw = phase & 1;
  const float* __restrict__ Bw = g.Bw + (size_t)phase * g.K * g.N;

  // ---------------- per-thread load geometry ----------------
  // A (CONV/CONVT2, vector): rows (tid>>3)+32i, quad tid&7
  constexpr int AR = BM / 32;
  long long abase[(MODE != MODE_WGRAD && AV) ? AR : 1];
  int aih[(MODE != MODE_WGRAD && AV) ? AR : 1], aiw[(MODE != MODE_WGRAD && AV) ? AR : 1];
  if constexpr (MODE != MODE_WGRAD && AV) {
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      int m = m0 + (tid >> 3) + 32 * i;
      if (m < g.M) {
        uint32_t b = g.fghw.div(m);
        uint32_t rem = m - b * g.fghw.d;
        uint32_t oi = g.fgw.div(rem);
        uint32_t oj = rem - oi * g.fgw.d;
        abase[i] = (long long)b * g.a.sb;
        if constexpr (MODE == MODE_CONV) {
          aih[i] = (int)oi * g.stride - g.pad;
          aiw[i] = (int)oj * g.stride - g.pad;
        } else {
          aih[i] = (int)oi;
          aiw[i] = (int)oj;
        }
      } else {
        abase[i] = 0;
        aih[i] = -(1 << 28);
        aiw[i] = 0;
      }
    }
  }
  // WGRAD B (vector): fixed column quad n = n0 + 4*(tid % (BN/4)) -> (kh, kw, ci)
  int wb_kh = 0, wb_kw = 0, wb_ci = 0;
  bool wb_nok = false;
  if constexpr (MODE == MODE_WGRAD && BV) {
    int n = n0 + 4 * (tid % (BN / 4));
    wb_nok = n < g.N;
    uint32_t t = g.fC.div(n);
    wb_ci = n - t * g.fC.d;
    wb_kh = g.fKW.div(t);
    wb_kw = t - wb_kh * g.fKW.d;
  }

  // register staging
  constexpr int A_ELEMS = BM * BK / 256;   // floats per thread
  constexpr int B_ELEMS = BK * BN / 256;
  float ra[A_ELEMS];
  float rb[B_ELEMS];

  // ---------------- FAST-path state ----------------
  static_assert(!FAST || (AV && BV), "FAST needs vector operands");
  // WGRAD FAST thread map (per operand of R rows = BM or BN): tid -> quad q = (tid&7) +
  // 8 ((tid>>5) % (R/32)), pixels p = ((tid>>3)&3) + 4 ((tid>>5) / (R/32)) + (32/(R/32)) i
  constexpr int FA_N = (MODE == MODE_WGRAD) ? BM / 32 : AR;  // A loads per thread
  constexpr int FB_N = BN / 32;
  auto sw_q = [&](int R) { return (tid & 7) + 8 * ((tid >> 5) % (R / 32)); };
  auto sw_p = [&](int R, int i) { return ((tid >> 3) & 3) + 4 * ((tid >> 5) / (R / 32)) + (32 / (R / 32)) * i; };
  // WGRAD FAST: im2col pixel offsets of the next tiles, per tap of the block's n tile (a
  // tile holds one tap when Cin >= BN, else BN / Cin <= 4 whole taps of one kernel row)
  __shared__ int ptab[2][4 * BK];
  __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc((void*)g.a.p, (short)0, g.a_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t brsrc =
      MODE == MODE_WGRAD ? __builtin_amdgcn_make_buffer_rsrc((void*)g.im.p, (short)0, g.im_bytes, 0x00020000)
                         : __builtin_amdgcn_make_buffer_rsrc((void*)Bw, (short)0, g.bw_bytes, 0x00020000);
  int aoff[FAST ? FA_N : 1], boff[FAST ? FB_N : 1];
  int f_tap = 0, f_c0 = 0, f_cin = 1, w_tab = 0;
  int w_ntap = 1, w_tq = 0, w_qb = 0;  // WGRAD FAST: taps per n tile; this thread's tap, channel byte offset
  int st_k0 = 0;                        // WGRAD FAST: first pixel row of the tile in the staging registers
  if constexpr (FAST) {
    if constexpr (MODE != MODE_WGRAD) {
      // packed weights [N][K]: rows n = n0 + (tid>>3) + 32i, k quad tid&7 (like A)
#pragma unroll
      for (int i = 0; i < FB_N; ++i) {
        const int n = n0 + (tid >> 3) + 32 * i;
        boff[i] = n < g.N ? (n * g.K + 4 * (tid & 7)) * 4 : OOB;
      }
      f_cin = g.fC.d;
      f_tap = kbeg / f_cin;
      f_c0 = kbeg - f_tap * f_cin;
    } else {
      const int m = m0 + 4 * sw_q(BM);
#pragma unroll
      for (int i = 0; i < FA_N; ++i) aoff[i] = m < g.M ? (sw_p(BM, i) * (int)g.a.sw + m) * 4 : OOB;
      // the block's n tile lies in one tap: n0 -> (kh, kw, ci0), wave-uniform
      const uint32_t t = g.fC.div(n0);
      const int ci0 = n0 - t * g.fC.d;
      const uint32_t kh = g.fKW.div(t);
      const int kw = t - kh * g.fKW.d;
      w_tab = ((int)kh - g.pad) * (int)g.im.sh + ((int)kw - g.pad) * (int)g.im.sw + ci0;  // tap part
      f_tap = (int)kh;   // kept for the bounds checks below
      f_c0 = kw;
      // column quad of this thread's B loads -> (tap within the tile, channel): with
      // Cin >= BN every quad is in the first tap (4 q < BN <= Cin)
      const int cin = (int)g.fC.d, c4 = 4 * sw_q(BN);
      w_ntap = cin >= BN ? 1 : BN / cin;
      w_tq = cin >= BN ? 0 : c4 / cin;
      w_qb = (c4 - w_tq * cin) * 4;
    }
  }
  // CONV/CONVT2 FAST: per-row offsets for the current tap
  auto set_tap = [&](int tap) {
    if constexpr (FAST && MODE != MODE_WGRAD) {
      int dh, dw;
      if constexpr (MODE == MODE_CONV) {
        dh = tap / g.KW;
        dw = tap - dh * g.KW;
      } else {
        dh = ph - (tap >> 1);
        dw = pw - (tap & 1);
      }
      const int q = tid & 7;
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const int ih = aih[i] + dh, iw = aiw[i] + dw;
        aoff[i] = ((unsigned)ih < (unsigned)g.a.H && (unsigned)iw < (unsigned)g.a.W)
                      ? ((int)abase[i] + ih * (int)g.a.sh + iw * (int)g.a.sw) * 4 + q * 16
                      : OOB;
      }
    }
  };
  // WGRAD FAST: one wave writes the im2col pixel offsets of tile k0 into ptab[slot], for
  // each of the tile's taps (kw0 + t of kernel row kh)
  auto build_table = [&](int k0, int slot) {
    if constexpr (FAST && MODE == MODE_WGRAD) {
      const int l = tid & 63;
      if (l < BK) {
        const int p = k0 + l;
        const uint32_t b = g.fghw.div(p);
        const uint32_t rem = p - b * g.fghw.d;
        const uint32_t oi = g.fgw.div(rem);
        const uint32_t oj = rem - oi * g.fgw.d;
        const int ih = (int)oi * g.stride - g.pad + f_tap;
        const int pix = (int)b * (int)g.im.sb + (int)oi * g.stride * (int)g.im.sh + (int)oj * g.stride * (int)g.im.sw;
        const bool rok = p < kend && (unsigned)ih < (unsigned)g.im.H;
        for (int t = 0; t < w_ntap; ++t) {
          const int iw = (int)oj * g.stride - g.pad + f_c0 + t;
          ptab[slot][t * BK + l] =
              (rok && (unsigned)iw < (unsigned)g.im.W) ? (pix + w_tab + t * (int)g.im.sw) * 4 : OOB;
        }
      }
    }
  };
  auto load_fast = [&](int k0, int slot) {
    if constexpr (FAST && MODE != MODE_WGRAD) {
      if (f_c0 == f_cin) {
        f_c0 = 0;
        set_tap(++f_tap);
      }
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(arsrc, aoff[i], f_c0 * 4, 0);
        ra[4 * i + 0] = __uint_as_float(v.x); ra[4 * i + 1] = __uint_as_float(v.y);
        ra[4 * i + 2] = __uint_as_float(v.z); ra[4 * i + 3] = __uint_as_float(v.w);
      }
      f_c0 += BK;
      const int so = k0 * 4;
#pragma unroll
      for (int i = 0; i < FB_N; ++i) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(brsrc, boff[i], so, 0);
        rb[4 * i + 0] = __uint_as_float(v.x); rb[4 * i + 1] = __uint_as_float(v.y);
        rb[4 * i + 2] = __uint_as_float(v.z); rb[4 * i + 3] = __uint_as_float(v.w);
      }
    } else if constexpr (FAST) {
      st_k0 = k0;
      const int so = k0 * (int)g.a.sw * 4;
#pragma unroll
      for (int i = 0; i < FA_N; ++i) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(arsrc, aoff[i], so, 0);
        ra[4 * i + 0] = __uint_as_float(v.x); ra[4 * i + 1] = __uint_as_float(v.y);
        ra[4 * i + 2] = __uint_as_float(v.z); ra[4 * i + 3] = __uint_as_float(v.w);
      }
#pragma unroll
      for (int i = 0; i < FB_N; ++i) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(brsrc, ptab[slot][w_tq * BK + sw_p(BN, i)] + w_qb, 0, 0);
        rb[4 * i + 0] = __uint_as_float(v.x); rb[4 * i + 1] = __uint_as_float(v.y);
        rb[4 * i + 2] = __uint_as_float(v.z); rb[4 * i + 3] = __uint_as_float(v.w);
      }
    }
  };

  auto load_tiles = [&](int k0) {
    // ---------------- A ----------------
    if constexpr (MODE != MODE_WGRAD) {
      if constexpr (AV) {
        const int q = tid & 7;
        const int k = k0 + 4 * q;
        int dh = 0, dw = 0, ci = 0;
        const bool kok = k < kend;
        if (kok) {
          uint32_t t = g.fC.div(k);
          ci = k - t * g.fC.d;
          if constexpr (MODE == MODE_CONV) {
            uint32_t kh = g.fKW.div(t);
            dh = kh;
            dw = t - kh * g.fKW.d;
          } else {
            int th = t >> 1, tw = t & 1;
            dh = ph - th;
            dw = pw - tw;
          }
        }
#pragma unroll
        for (int i = 0; i < AR; ++i) {
          int ih = aih[i] + dh, iw = aiw[i] + dw;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (kok && (unsigned)ih < (unsigned)g.a.H && (unsigned)iw < (unsigned)g.a.W)
            v = *reinterpret_cast<const float4*>(g.a.p + abase[i] + (long long)ih * g.a.sh +
                                                 (long long)iw * g.a.sw + ci);
          ra[4 * i + 0] = v.x; ra[4 * i + 1] = v.y; ra[4 * i + 2] = v.z; ra[4 * i + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < A_ELEMS; ++j) {
          int e = tid + 256 * j;
          int row = e >> 5, col = e & 31;
          int m = m0 + row, k = k0 + col;
          float v = 0.f;
          if (m < g.M && k < kend) {
            uint32_t b = g.fghw.div(m);
            uint32_t rem = m - b * g.fghw.d;
            uint32_t oi = g.fgw.div(rem);
            uint32_t oj = rem - oi * g.fgw.d;
            uint32_t t = g.fC.div(k);
            int ci = k - t * g.fC.d;
            int ih, iw;
            if constexpr (MODE == MODE_CONV) {
              uint32_t kh = g.fKW.div(t);
              ih = (int)oi * g.stride - g.pad + (int)kh;
              iw = (int)oj * g.stride - g.pad + (int)(t - kh * g.fKW.d);
            } else {
              ih = (int)oi + ph - (int)(t >> 1);
              iw = (int)oj + pw - (int)(t & 1);
            }
            if ((unsigned)ih < (unsigned)g.a.H && (unsigned)iw < (unsigned)g.a.W)
              v = g.a.p[(long long)b * g.a.sb + (long long)ih * g.a.sh + (long long)iw * g.a.sw +
                        (long long)ci * g.a.sc];
          }
          ra[j] = v;
        }
      }
    } else {
      // WGRAD A: rows p (k dim), cols m (gradient channel)
      if constexpr (AV) {
        constexpr int TPR = BM / 4, RPP = 256 / TPR, PASSES = BK / RPP;
        const int q = tid % TPR, r = tid / TPR;
        const int m = m0 + 4 * q;
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
          int p = k0 + r + RPP * i;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (p < kend && m < g.M) {
            uint32_t b = g.fghw.div(p);
            uint32_t rem = p - b * g.fghw.d;
            uint32_t oi = g.fgw.div(rem);
            uint32_t oj = rem - oi * g.fgw.d;
            v = *reinterpret_cast<const float4*>(g.a.p + (long long)b * g.a.sb + (long long)oi * g.a.sh +
                                                 (long long)oj * g.a.sw + m);
          }
          ra[4 * i + 0] = v.x; ra[4 * i + 1] = v.y; ra[4 * i + 2] = v.z; ra[4 * i + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < A_ELEMS; ++j) {
          int e = tid + 256 * j;
          int row = e / BM, col = e - (e / BM) * BM;
          int p = k0 + row, m = m0 + col;
          float v = 0.f;
          if (p < kend && m < g.M) {
            uint32_t b = g.fghw.div(p);
            uint32_t rem = p - b * g.fghw.d;
            uint32_t oi = g.fgw.div(rem);
            uint32_t oj = rem - oi * g.fgw.d;
            v = g.a.p[(long long)b * g.a.sb + (long long)oi * g.a.sh + (long long)oj * g.a.sw +
                      (long long)m * g.a.sc];
          }
          ra[j] = v;
        }
      }
    }
    // ---------------- B ----------------
    if constexpr (MODE != MODE_WGRAD) {
      // packed weights [N][K]: k fastest across threads (coalesced), staged [k][n]
#pragma unroll
      for (int j = 0; j < B_ELEMS; ++j) {
        int e = tid + 256 * j;
        int row = e / BK, col = e - row * BK;
        int k = k0 + col, n = n0 + row;
        rb[j] = (k < kend && n < g.N) ? Bw[(size_t)n * g.K + k] : 0.f;
      }
    } else {
      // WGRAD B: im2col(img)[p][n]
      if constexpr (BV) {
        constexpr int TPR = BN / 4, RPP = 256 / TPR, PASSES = BK / RPP;
        const int r = tid / TPR;
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
          int p = k0 + r + RPP * i;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (p < kend && wb_nok) {
            uint32_t b = g.fghw.div(p);
            uint32_t rem = p - b * g.fghw.d;
            uint32_t oi = g.fgw.div(rem);
            uint32_t oj = rem - oi * g.fgw.d;
            int ih = (int)oi * g.stride - g.pad + wb_kh;
            int iw = (int)oj * g.stride - g.pad + wb_kw;
            if ((unsigned)ih < (unsigned)g.im.H && (unsigned)iw < (unsigned)g.im.W)
              v = *reinterpret_cast<const float4*>(g.im.p + (long long)b * g.im.sb + (long long)ih * g.im.sh +
                                                   (long long)iw * g.im.sw + wb_ci);
          }
          rb[4 * i + 0] = v.x; rb[4 * i + 1] = v.y; rb[4 * i + 2] = v.z; rb[4 * i + 3] = v.w;
        }
      } else {
        if (g.im_buf) {
          // every gather unconditional, a tap outside the image at an offset past the
          // descriptor (reads 0): a conditional load compiles into a branch that waits for it
          // -- one gather in flight per thread (round 6: C4's input-layer weight gradient)
#pragma unroll
          for (int j = 0; j < B_ELEMS; ++j) {
            const int e = tid + 256 * j, row = e / BN, col = e - row * BN, p = k0 + row, n = n0 + col;
            const bool in = p < kend && n < g.N;
            const uint32_t b = g.fghw.div(p), rem = p - b * g.fghw.d, oi = g.fgw.div(rem), oj = rem - oi * g.fgw.d;
            const uint32_t t = g.fC.div(n), kh = g.fKW.div(t);
            const int ci = n - t * g.fC.d, kw = t - kh * g.fKW.d;
            const int ih = (int)oi * g.stride - g.pad + (int)kh, iw = (int)oj * g.stride - g.pad + kw;
            const bool ok = in && (unsigned)ih < (unsigned)g.im.H && (unsigned)iw < (unsigned)g.im.W;
            const int off = (int)b * (int)g.im.sb + ih * (int)g.im.sh + iw * (int)g.im.sw + ci * (int)g.im.sc;
            rb[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(brsrc, ok ? 4 * off : 0x7ffffff0, 0, 0));
          }
        } else {
#pragma unroll
          for (int j = 0; j < B_ELEMS; ++j) {
            int e = tid + 256 * j;
            int row = e / BN, col = e - (e / BN) * BN;
            int p = k0 + row, n = n0 + col;
            float v = 0.f;
            if (p < kend && n < g.N) {
              uint32_t b = g.fghw.div(p);
              uint32_t rem = p - b * g.fghw.d;
              uint32_t oi = g.fgw.div(rem);
              uint32_t oj = rem - oi * g.fgw.d;
              uint32_t t = g.fC.div(n);
              int ci = n - t * g.fC.d;
              uint32_t kh = g.fKW.div(t);
              int kw = t - kh * g.fKW.d;
              int ih = (int)oi * g.stride - g.pad + (int)kh;
              int iw = (int)oj * g.stride - g.pad + kw;
              if ((unsigned)ih < (unsigned)g.im.H && (unsigned)iw < (unsigned)g.im.W)
                v = g.im.p[(long long)b * g.im.sb + (long long)ih * g.im.sh + (long long)iw * g.im.sw +
                           (long long)ci * g.im.sc];
            }
            rb[j] = v;
          }
        }
      }
    }
  };

  // bias gradient of a FAST conv WGRAD (GemmArgs::dbias): this thread's 4 channels (m0 + 4 q
  // .. + 3, q = sw_q(BM)) summed in double over the pixels it stages
  const bool db_on = SWZ && g.dbias != nullptr && tn_i == 0;
  double dbs[4] = {0.0, 0.0, 0.0, 0.0};
  auto store_tiles = [&](int buf) {
    float* As = smem + buf * STAGE;
    float* Bs = As + A_SZ;
    if constexpr (SWZ) {
      if (db_on && st_k0 >= g.db_k0) {  // tile-uniform: db_k0 is a multiple of BK
#pragma unroll
        for (int i = 0; i < FA_N; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) dbs[j] += (double)ra[4 * i + j];
      }
      // element (row, k) at row * 32 + 4 ((k >> 2) ^ ((row >> 1) & 7)) + (k & 3)
      auto put = [&](float* T, int R, const float* v, int nld) {
        const int q = sw_q(R);
#pragma unroll
        for (int i = 0; i < nld; ++i) {
          const int k = sw_p(R, i);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int row = 4 * q + j;
            T[row * KROW_LD + 4 * ((k >> 2) ^ ((row >> 1) & 7)) + (k & 3)] = v[4 * i + j];
          }
        }
      };
      put(As, BM, ra, FA_N);
      put(Bs, BN, rb, FB_N);
      return;
    } else if constexpr (KROW) {
      const int q = tid & 7;
#pragma unroll
      for (int i = 0; i < AR; ++i)
        *reinterpret_cast<float4*>(As + ((tid >> 3) + 32 * i) * KROW_LD + 4 * q) =
            make_float4(ra[4 * i], ra[4 * i + 1], ra[4 * i + 2], ra[4 * i + 3]);
#pragma unroll
      for (int i = 0; i < FB_N; ++i)
        *reinterpret_cast<float4*>(Bs + ((tid >> 3) + 32 * i) * KROW_LD + 4 * q) =
            make_float4(rb[4 * i], rb[4 * i + 1], rb[4 * i + 2], rb[4 * i + 3]);
      return;
    }
    if constexpr (MODE != MODE_WGRAD) {
      if constexpr (AV) {
        const int q = tid & 7;
#pragma unroll
        for (int i = 0; i < AR; ++i) {
          float* dst = As + ((tid >> 3) + 32 * i) * A_LD + 4 * q;
          dst[0] = ra[4 * i + 0]; dst[1] = ra[4 * i + 1]; dst[2] = ra[4 * i + 2]; dst[3] = ra[4 * i + 3];
        }
      } else {
#pragma unroll
        for (int j = 0; j < A_ELEMS; ++j) {
          int e = tid + 256 * j;
          As[(e >> 5) * A_LD + (e & 31)] = ra[j];
        }
      }
    } else {
      if constexpr (AV) {
        constexpr int TPR = BM / 4, RPP = 256 / TPR, PASSES = BK / RPP;
        const int q = tid % TPR, r = tid / TPR;
#pragma unroll
        for (int i = 0; i < PASSES; ++i)
          *reinterpret_cast<float4*>(As + (r + RPP * i) * A_LD + 4 * q) =
              make_float4(ra[4 * i], ra[4 * i + 1], ra[4 * i + 2], ra[4 * i + 3]);
      } else {
#pragma unroll
        for (int j = 0; j < A_ELEMS; ++j) {
          int e = tid + 256 * j;
          int row = e / BM;
          As[row * A_LD + (e - row * BM)] = ra[j];
        }
      }
    }
    if constexpr (MODE != MODE_WGRAD) {  // [N][K] weights, k fastest (load_tiles)
#pragma unroll
      for (int j = 0; j < B_ELEMS; ++j) {
        int e = tid + 256 * j;
        int row = e / BK;
        Bs[(e - row * BK) * B_LD + row] = rb[j];
      }
    } else if constexpr (BV) {
      constexpr int TPR = BN / 4, RPP = 256 / TPR, PASSES = BK / RPP;
      const int q = tid % TPR, r = tid / TPR;
#pragma unroll
      for (int i = 0; i < PASSES; ++i)
        *reinterpret_cast<float4*>(Bs + (r + RPP * i) * B_LD + 4 * q) =
            make_float4(rb[4 * i], rb[4 * i + 1], rb[4 * i + 2], rb[4 * i + 3]);
    } else {
#pragma unroll
      for (int j = 0; j < B_ELEMS; ++j) {
        int e = tid + 256 * j;
        int row = e / BN;
        Bs[row * B_LD + (e - row * BN)] = rb[j];
      }
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // vector epilogue's per-tile output row offsets (FAST 64x64-per-wave tiles)
  constexpr bool VEC_EPI = KROW && BM / WM == 64 && BN / WN == 64;
  __shared__ long long emoff[VEC_EPI ? BM : 1];
  // Producer post-op (gemm_post: unsplit tiles, vector epilogue): the rows of px the epilogue
  // multiplies by are loaded into registers at the start of the LAST k tile, so their HBM
  // latency hides under that tile's MFMAs instead of stalling the epilogue.  The row-offset
  // table they index is written here, at the start, and published by the main loop's barriers.
  float4 pax[VEC_EPI && POST ? 16 : 1];
  const bool post_pf = POST && VEC_EPI && g.pmode && g.splits == 1 && g.vec_out;
  if constexpr (POST && VEC_EPI) {
    if (post_pf) {
      for (int i = tid; i < BM; i += 256) {
        const int m = m0 + i;
        emoff[i] = m < g.M ? row_offset(g.out, m, MODE == MODE_CONVT2 ? phase : 0) : 0;
      }
    }
  }
  auto post_prefetch = [&]() {
    if constexpr (POST && VEC_EPI) {
      const int n = n0 + wn + 4 * (lane & 15);
      if (post_pf && n < g.N) {
        const long long noff = col_offset(g.out, n);
#pragma unroll
        for (int s4 = 0; s4 < 16; ++s4) {
          const int rl = 4 * s4 + (lane >> 4), m = m0 + wm + rl;
          pax[s4] = m < g.M ? *reinterpret_cast<const float4*>(g.px + emoff[wm + rl] + noff)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
    }
  };

  if constexpr (FAST && MODE == MODE_WGRAD) {
    if (wid == 0) build_table(kbeg, 0);
    if (wid == 1 && nk > 1) build_table(kbeg + BK, 1);
    __syncthreads();
  }
  if constexpr (FAST && MODE != MODE_WGRAD) set_tap(f_tap);
  const int l32 = lane & 31, lk = lane >> 5;
  if constexpr (EMU) {
    // fp32 GEMM on the bf16 MFMA: every operand is split EXACTLY into three bf16 pieces
    // (x = hi + mid + lo, 8 significant bits each: hi = x with the low 16 bits cleared,
    // mid likewise of x - hi, lo = x - hi - mid, exact in bf16), and each product keeps the
    // six terms down to 2^-16 relative: hh, hm, mh, hl, lh, mm (bf16 x bf16 products are
    // exact in fp32; the dropped ml, lm, ll terms are <= 2^-23 relative -- one fp32
    // rounding).  v_mfma_f32_32x32x16_bf16 has 16x the rate of the fp32 MFMA, so 6 of them
    // are 2.67x fewer MFMA cycles; the split (about 6 VALU per element) overlaps the bf16
    // MFMAs, which -- unlike fp32 MFMA -- co-execute with VALU.
    typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
    uint32_t* P = reinterpret_cast<uint32_t*>(smem);  // planes 0-2 A, 3-5 B
    auto split_store = [&](uint32_t* base, int row, int q, const float* v) {
      uint32_t h[4], m[4], l[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t xb = __float_as_uint(v[e]);
        h[e] = xb & 0xffff0000u;
        const float r1 = v[e] - __uint_as_float(h[e]);
        m[e] = __float_as_uint(r1) & 0xffff0000u;
        l[e] = __float_as_uint(r1 - __uint_as_float(m[e]));
      }
      const int o = row * EMU_RS + 2 * q;  // k 4q .. 4q+3 = dwords 2q, 2q+1 of the row
      *reinterpret_cast<uint2*>(base + o) = make_uint2((h[0] >> 16) | h[1], (h[2] >> 16) | h[3]);
      *reinterpret_cast<uint2*>(base + EMU_PLANE + o) = make_uint2((m[0] >> 16) | m[1], (m[2] >> 16) | m[3]);
      *reinterpret_cast<uint2*>(base + 2 * EMU_PLANE + o) =
          make_uint2((l[0] >> 16) | (l[1] & 0xffff0000u), (l[2] >> 16) | (l[3] & 0xffff0000u));
    };
    auto store_emu = [&]() {
      const int q = tid & 7;
#pragma unroll
      for (int i = 0; i < AR; ++i) split_store(P, (tid >> 3) + 32 * i, q, ra + 4 * i);
#pragma unroll
      for (int i = 0; i < FB_N; ++i) split_store(P + 3 * EMU_PLANE, (tid >> 3) + 32 * i, q, rb + 4 * i);
    };
    if (nk > 0) {
      load_fast(kbeg, 0);
      store_emu();
    }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      // registers only, in flight during the MFMAs.  Unconditional: a guarded load leaves
      // the compiler a phi of (new, old) registers whose copies wait for the loads right
      // here.  Past the last tile every offset is in-bounds or OOB (buffer loads return 0).
      load_fast(kbeg + (kt + 1) * BK, 0);
      if (kt + 1 == nk) post_prefetch();
      __builtin_amdgcn_sched_barrier(0);  // keep the loads ahead of the MFMAs (not sunk for VGPRs)
#pragma unroll
      for (int t = 0; t < 2; ++t) {  // two k16 steps per BK = 32 tile; lane half lk takes k 8 lk .. 8 lk + 7
        bf16x8 af[3][TM], bfr[3][TN];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
          for (int i = 0; i < TM; ++i)
            af[pl][i] = *reinterpret_cast<const bf16x8*>(P + pl * EMU_PLANE + (wm + 32 * i + l32) * EMU_RS + 8 * t + 4 * lk);
#pragma unroll
          for (int j = 0; j < TN; ++j)
            bfr[pl][j] = *reinterpret_cast<const bf16x8*>(P + (3 + pl) * EMU_PLANE + (wn + 32 * j + l32) * EMU_RS +
                                                          8 * t + 4 * lk);
        }
        // (A first: rows of the product are pixels, columns output channels, as in the fp32 path)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            f32x16 c = acc[i][j];
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][i], bfr[2][j], c, 0, 0, 0);  // A hi x B lo
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2][i], bfr[0][j], c, 0, 0, 0);  // A lo x B hi
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1][i], bfr[1][j], c, 0, 0, 0);  // A mid x B mid
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][i], bfr[1][j], c, 0, 0, 0);  // A hi x B mid
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1][i], bfr[0][j], c, 0, 0, 0);  // A mid x B hi
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][i], bfr[0][j], c, 0, 0, 0);  // A hi x B hi
          }
      }
      __syncthreads();  // every wave's reads of this tile are done
      if (kt + 1 < nk) {
        store_emu();
        __syncthreads();
      }
    }
  } else {
  if (nk > 0) {
    if constexpr (FAST) load_fast(kbeg, 0);
    else load_tiles(kbeg);
    store_tiles(0);
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = GEMM_SB ? 0 : kt & 1;
    if (kt + 1 < nk) {
      if constexpr (FAST) load_fast(kbeg + (kt + 1) * BK, (kt + 1) & 1);
      else load_tiles(kbeg + (kt + 1) * BK);
    } else {
      post_prefetch();
    }
    if constexpr (FAST && MODE == MODE_WGRAD) {
      if (kt + 2 < nk && wid == (kt & 3)) build_table(kbeg + (kt + 2) * BK, kt & 1);
    }
    const float* As = smem + cur * STAGE;
    const float* Bs = As + A_SZ;
    if constexpr (KROW) {
      // logical quad g = kq + 4 lk of row wm/wn + 32 t + l32; SWZ: physical quad g ^ swz
      // with swz = (l32 >> 1) & 7 (wm, wn, 32 t are multiples of 32)
      const int swz = SWZ ? (l32 >> 1) & 7 : 0;
      const float* Ar = As + (wm + l32) * KROW_LD;
      const float* Br = Bs + (wn + l32) * KROW_LD;
#pragma unroll
      for (int kq = 0; kq < BK / 8; ++kq) {
        const int qo = 4 * ((kq + 4 * lk) ^ swz);
        float4 a4[TM], b4[TN];
#pragma unroll
        for (int t = 0; t < TM; ++t) a4[t] = *reinterpret_cast<const float4*>(Ar + 32 * t * KROW_LD + qo);
#pragma unroll
        for (int t = 0; t < TN; ++t) b4[t] = *reinterpret_cast<const float4*>(Br + 32 * t * KROW_LD + qo);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[i][s4], b4[j][s4], acc[i][j], 0, 0, 0);
      }
    } else {
    // per-lane base pointers: every operand read below is base + compile-time offset,
    // which folds into the DS instruction's immediate (no per-read address VALU)
    const float* Al = AK ? As + lk * A_LD + wm + l32 : As + (wm + l32) * A_LD + lk;
    const float* Bl = Bs + lk * B_LD + wn + l32;
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      float af[TM], bf[TN];
#pragma unroll
      for (int t = 0; t < TM; ++t) af[t] = AK ? Al[2 * kk * A_LD + 32 * t] : Al[32 * t * A_LD + 2 * kk];
#pragma unroll
      for (int t = 0; t < TN; ++t) bf[t] = Bl[2 * kk * B_LD + 32 * t];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    }
    if constexpr (GEMM_SB) {
      if (kt + 1 < nk) {
        __syncthreads();  // every wave's reads of the one stage are done
        store_tiles(0);
      }
    } else if (kt + 1 < nk) {
      store_tiles(cur ^ 1);
    }
    __syncthreads();
  }
  }  // EMU / fp32 main loop

  const bool split_out = g.splits > 1;  // partial sums for a separate splitk_reduce

  if constexpr (SWZ) {
    if (db_on) {
      // the NT8 = 1024 / BM threads staging the same channel quad (pixel slots t8 =
      // ((tid >> 3) & 3) + 4 ((tid >> 5) / (BM / 32)): 8 slots for 128-row tiles, 16 for the
      // 64-row ones) -> one double per channel, t8 in order (the main loop's last barrier has
      // retired every stage read; the epilogue reuses smem after the second barrier)
      double* dsh = reinterpret_cast<double*>(smem);
      constexpr int NT8 = 1024 / BM;  // threads staging one channel quad
      const int q = sw_q(BM), t8 = ((tid >> 3) & 3) + 4 * ((tid >> 5) / (BM / 32));
#pragma unroll
      for (int j = 0; j < 4; ++j) dsh[t8 * BM + 4 * q + j] = dbs[j];
      __syncthreads();
      if (tid < BM && m0 + tid < g.M) {
        double v = 0.0;
#pragma unroll
        for (int t = 0; t < NT8; ++t) v += dsh[t * BM + tid];
        if (split_out) {
          g.dbp[(size_t)split * g.M + m0 + tid] = v;
        } else {
          float* dst = g.dbias + m0 + tid;
          *dst = g.db_accum ? *dst + (float)v : (float)v;
        }
      }
      __syncthreads();
    }
  }

  // ---------------- epilogue ----------------
  if constexpr (VEC_EPI) {
    // Vector epilogue (FAST, 64x64 per wave): each wave stages its finished sub-tile in LDS
    // (row stride 72: the two lane halves' rows 4 apart land 32 banks apart) and writes it
    // back as float4 rows -- 16 b128 stores per lane instead of 64 scalar ones, 256
    // contiguous bytes per output row.  The scalar stores' bursts at the end of every tile
    // (all blocks finish together) held the MFMA pipes idle on short-K layers.
    const bool slab_out = split_out;
    if ((slab_out && g.N % 4 == 0) || (!slab_out && g.vec_out)) {
      constexpr int EP_LD = 72, EPR = GEMM_SB ? 32 : 64, NP = 64 / EPR;
      float* T = smem + wid * (EPR * EP_LD);
      const float wsc = (!slab_out && g.wscale) ? g.wscale[0] : 1.f;
      if (!slab_out && !post_pf) {
        for (int i = tid; i < BM; i += 256) {
          const int m = m0 + i;
          emoff[i] = m < g.M ? row_offset(g.out, m, MODE == MODE_CONVT2 ? phase : 0) : 0;
        }
      }
      // the activation branch is taken once per tile (uniform), not once per element
      auto stage = [&](auto actf, int pp) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int cl = 32 * j + l32, col = n0 + wn + cl;
          const float bv = (!slab_out && g.bias && col < g.N) ? g.bias[col] : 0.f;
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            if (NP > 1 && i != pp) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int rl = 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk - EPR * pp;
              T[rl * EP_LD + cl] = actf(acc[i][j][r] * wsc + bv);
            }
          }
        }
      };
      const bool bn_stats = !slab_out && g.bnp;
      double s1 = 0.0, s2 = 0.0;
      const int q = lane & 15, n = n0 + wn + 4 * q;
      float* slab = slab_out ? g.slab + (size_t)z * g.M * g.N : nullptr;
      const long long noff = (slab_out || n >= g.N) ? 0 : col_offset(g.out, n);
      // producer post-op (unsplit only; the reduce applies it to split tiles).  pmode 2: the
      // wave's 64 rows are one 64-row segment of one batch segment (host: bn_post_ok)
      const int pmode = (!POST || slab_out) ? 0 : g.pmode;
      float p_al[4], p_be[4], p_mu[4];
      double p1[4] = {0.0, 0.0, 0.0, 0.0}, p2[4] = {0.0, 0.0, 0.0, 0.0};
      if (pmode == 2) {
        const int k = post_seg(g, m0 + wm);
#pragma unroll
        for (int i = 0; i < 4; ++i) post_consts(g, k, n + i, p_al[i], p_be[i], p_mu[i]);
      }
#pragma unroll
      for (int pp = 0; pp < NP; ++pp) {
        if (pp > 0) __syncthreads();  // the previous pass's T reads are done
        if (slab_out || g.act <= RGAN_ACT_LRELU) {
          const float neg = (slab_out || g.act == RGAN_ACT_NONE) ? 1.f : (g.act == RGAN_ACT_RELU ? 0.f : g.alpha);
          stage([neg](float v) { return v > 0.f ? v : v * neg; }, pp);
        } else {
          stage([&](float v) { return act_fwd_curved(v, g.act, g.alpha); }, pp);
        }
        __syncthreads();
        if (bn_stats) {
          // BatchNorm batch statistics in the epilogue: the wave's finished rows of column
          // `lane` (one channel; conflict-free LDS row reads) -> (sum y, sum y^2) of the
          // 64-row segment in double, rows in order (fp32 products are exact in double; the
          // merge is a plain fixed-order sum).  Host guarantees M % 64 == 0 and n == channel;
          // segment = (phase, m / 64).
#pragma unroll 8
          for (int rl = 0; rl < EPR; ++rl) {
            const double d = (double)T[rl * EP_LD + lane];
            s1 += d;
            s2 += d * d;
          }
        }
        if (n < g.N && pmode) {
          // producer post-op: the wave's 16 rows of px, loaded during the last k tile
          // (post_prefetch; GEMM_SB is off for these 128x128 tiles: one pass, pp = 0)
          static_assert(!POST || EPR == 64, "post-op prefetch covers one 64-row pass");
          const float4* ax = pax;
#pragma unroll
          for (int s4 = 0; s4 < EPR / 4; ++s4) {
            const int rl = 4 * s4 + (lane >> 4), m = m0 + wm + EPR * pp + rl;
            if (m < g.M) {
              const float4 v = *reinterpret_cast<const float4*>(T + rl * EP_LD + 4 * q);
              float vv[4] = {v.x, v.y, v.z, v.w};
              const float aa[4] = {ax[s4].x, ax[s4].y, ax[s4].z, ax[s4].w};
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                if (pmode == 1) {
                  vv[i] *= act_grad_from_out(aa[i], g.pact, g.palpha);
                } else {
                  vv[i] *= act_grad_from_in(aa[i] * p_al[i] + p_be[i], g.pact, g.palpha);
                  p1[i] += (double)vv[i];
                  p2[i] += (double)vv[i] * (double)(aa[i] - p_mu[i]);
                }
              }
              *reinterpret_cast<float4*>(g.C + emoff[wm + EPR * pp + rl] + noff) = make_float4(vv[0], vv[1], vv[2], vv[3]);
            }
          }
        } else if (n < g.N) {
#pragma unroll
          for (int s4 = 0; s4 < EPR / 4; ++s4) {
            const int rl = 4 * s4 + (lane >> 4), m = m0 + wm + EPR * pp + rl;
            if (m < g.M) {
              const float4 v = *reinterpret_cast<const float4*>(T + rl * EP_LD + 4 * q);
              float* dst = slab_out ? slab + (size_t)m * g.N + n : g.C + emoff[wm + EPR * pp + rl] + noff;
              *reinterpret_cast<float4*>(dst) = v;
            }
          }
        }
      }
      if (bn_stats) {
        const int mrow = m0 + wm, col = n0 + wn + lane;
        if (mrow < g.M && col < g.N) {
          const size_t seg = (size_t)phase * (uint32_t)(g.M >> 6) + (uint32_t)(mrow >> 6);
          g.bnp[(seg * 2) * g.N + col] = s1;
          g.bnp[(seg * 2 + 1) * g.N + col] = s2;
        }
      }
      if (pmode == 2) {
        // the 4 row groups (lane >> 4) of each column quad: fixed xor-butterfly (a + b == b + a
        // bitwise, so every lane of a group ends with the same sums)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          p1[i] += __shfl_xor(p1[i], 16);
          p2[i] += __shfl_xor(p2[i], 16);
          p1[i] += __shfl_xor(p1[i], 32);
          p2[i] += __shfl_xor(p2[i], 32);
        }
        const int mrow = m0 + wm;
        if ((lane >> 4) == 0 && mrow < g.M) {
          const size_t seg = (size_t)phase * (uint32_t)(g.M >> 6) + (uint32_t)(mrow >> 6);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (n + i < g.N) {
              g.ppart[(seg * 2) * g.N + n + i] = p1[i];
              g.ppart[(seg * 2 + 1) * g.N + n + i] = p2[i];
            }
          }
        }
      }
      return;
    }
  }
  if (split_out) {
    float* slab = g.slab + (size_t)z * g.M * g.N;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = n0 + wn + 32 * j + l32;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
          if (row < g.M && col < g.N) slab[(size_t)row * g.N + col] = acc[i][j][r];
        }
      }
    return;
  }
  const float wsc = g.wscale ? g.wscale[0] : 1.f;
  long long* moff = reinterpret_cast<long long*>(smem);
  long long* noff = moff + BM;
  for (int i = tid; i < BM; i += 256) {
    int m = m0 + i;
    moff[i] = m < g.M ? row_offset(g.out, m, MODE == MODE_CONVT2 ? phase : 0) : 0;
  }
  for (int i = tid; i < BN; i += 256) {
    int n = n0 + i;
    noff[i] = n < g.N ? col_offset(g.out, n) : 0;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int cl = wn + 32 * j + l32;
      const int col = n0 + cl;
      const float bv = (g.bias && col < g.N) ? g.bias[col] : 0.f;
      auto put = [&](auto actf) {
        if constexpr (MODE == MODE_WGRAD) {
          // accumulating: the 16 old values first, all in flight, through a descriptor over
          // dW (rows outside the tile at an offset past it) -- the read-modify-write per
          // element compiled into 16 dependent round trips
          if (g.accum && (long long)g.M * g.N * 4 < 0x7ffffff0LL) {
            const __amdgpu_buffer_rsrc_t crs =
                __builtin_amdgcn_make_buffer_rsrc((void*)g.C, (short)0, (int)(4LL * g.M * g.N), 0x00020000);
            float old[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int rl = wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
              const bool ok = m0 + rl < g.M && col < g.N;
              old[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                  crs, ok ? (int)(4 * (moff[rl] + noff[cl])) : 0x7ffffff0, 0, 0));
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int rl = wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
              if (m0 + rl < g.M && col < g.N) g.C[moff[rl] + noff[cl]] = old[r] + actf(acc[i][j][r] * wsc + bv);
            }
            return;
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rl = wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
          if (m0 + rl < g.M && col < g.N) {
            float v = acc[i][j][r] * wsc + bv;
            float* dst = g.C + moff[rl] + noff[cl];
            v = actf(v);
            *dst = (MODE == MODE_WGRAD && g.accum) ? *dst + v : v;
          }
        }
      };
      if (g.act <= RGAN_ACT_LRELU) {
        const float neg = g.act == RGAN_ACT_NONE ? 1.f : (g.act == RGAN_ACT_RELU ? 0.f : g.alpha);
        put([neg](float v) { return v > 0.f ? v : v * neg; });
      } else {
        put([&](float v) { return act_fwd_curved(v, g.act, g.alpha); });
      }
    }
  if constexpr (BM == 64 && BN == 64 && MODE != MODE_WGRAD) {
    if (g.bnp) {
      // BatchNorm segment sums of the 64 x 64 tile (unsplit, act none, n = channel, M % 64 ==
      // 0: host bn_epilogue_ok): the tile's 64 rows are one segment.  Per column: the lane's 16
      // rows in register order, then the two lane halves (xor 32), then the two waves of the
      // column (wm = 0, 32) in order through LDS -- (sum y, sum y^2) in double of the values
      // stored above, as the 128 x 128 vector epilogue writes them.
      double s1 = 0.0, s2 = 0.0;
      const int cl = wn + l32, col = n0 + cl;
      const float bv = (g.bias && col < g.N) ? g.bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const double d = (double)(acc[0][0][r] * wsc + bv);
        s1 += d;
        s2 += d * d;
      }
      s1 += __shfl_xor(s1, 32);
      s2 += __shfl_xor(s2, 32);
      double* bsh = reinterpret_cast<double*>(noff + BN);  // [2 waves][2][64]
      if (lk == 0) {
        bsh[(wm / 32) * 128 + cl] = s1;
        bsh[(wm / 32) * 128 + 64 + cl] = s2;
      }
      __syncthreads();
      if (tid < 64 && n0 + tid < g.N && m0 < g.M) {
        const size_t seg = (size_t)phase * (uint32_t)(g.M >> 6) + (uint32_t)(m0 >> 6);
        g.bnp[(seg * 2) * g.N + n0 + tid] = bsh[tid] + bsh[128 + tid];
        g.bnp[(seg * 2 + 1) * g.N + n0 + tid] = bsh[64 + tid] + bsh[192 + tid];
      }
    }
  }
}

template <int MODE, int BM, int BN, int WM, int WN, bool AV, bool BV, bool FAST>
__global__ __launch_bounds__(256, 2) void gemm_kernel(GemmArgs g) {
  gemm_body<MODE, BM, BN, WM, WN, AV, BV, FAST, false>(g);
}

// The FAST 128 x 128 CONV / CONVT2 GEMM with a producer post-op in its vector epilogue
// (GemmArgs::pmode, rgan_conv_post): its own instantiation, so the plain GEMMs' registers and
// schedule stay those of the post-free epilogue.
template <int MODE>
__global__ __launch_bounds__(256, 2) void gemm_post(GemmArgs g) {
  gemm_body<MODE, 128, 128, 2, 2, true, true, true, false, true>(g);
}
// ... and with the opt-in fp32-on-bf16x6 products (rgan_set_gemm_emulation)
template <int MODE>
__global__ __launch_bounds__(256, 2) void gemm_post_bf16x6(GemmArgs g) {
  gemm_body<MODE, 128, 128, 2, 2, true, true, true, true, true>(g);
}

// Opt-in (rgan_set_gemm_emulation): the FAST 128 x 128 CONV / CONVT2 GEMM with fp32 products
// emulated on the bf16 MFMA (see gemm_body's EMU path).  Its own symbol, reported as such.
template <int MODE>
__global__ __launch_bounds__(256, 2) void gemm_bf16x6(GemmArgs g) {
  gemm_body<MODE, 128, 128, 2, 2, true, true, true, true>(g);
}

// ---------------------------------------------------------------- launch
// One instantiation: its launch and the name it is reported under, from the same template arguments.
template <int MODE, int BM, int BN, int WM, int WN, bool AV, bool BV, bool FAST>
static void launch_gemm(const GemmLaunch& l) {
  auto tf = [](bool b) { return b ? "true" : "false"; };
  prof_kernel("void rgan::gemm_kernel<%d, %d, %d, %d, %d, %s, %s, %s>(rgan::GemmArgs)", MODE, BM, BN, WM, WN, tf(AV),
              tf(BV), tf(FAST));
  gemm_kernel<MODE, BM, BN, WM, WN, AV, BV, FAST><<<l.grid, 256, 0, l.s>>>(l.g);
}

template <int MODE, int BM, int BN, int WM, int WN>
static void launch_cfg(const GemmLaunch& l) {
  if (l.fast) launch_gemm<MODE, BM, BN, WM, WN, true, true, true>(l);
  else if (l.av && l.bv) launch_gemm<MODE, BM, BN, WM, WN, true, true, false>(l);
  else if (l.av) launch_gemm<MODE, BM, BN, WM, WN, true, false, false>(l);
  else if (l.bv) launch_gemm<MODE, BM, BN, WM, WN, false, true, false>(l);
  else launch_gemm<MODE, BM, BN, WM, WN, false, false, false>(l);
}

template <int MODE>
static void launch_mode(const GemmLaunch& l) {
  if constexpr (MODE == MODE_CONV || MODE == MODE_CONVT2) {
    // FAST 128x128 CONV / CONVT2 GEMMs (fwd + dgrad of Conv and ConvT) on the bf16x6 emulation: opt-in
    // by rgan_set_gemm_emulation (read at every launch: a captured graph keeps its kernels)
    const bool emu = l.fast && l.cfg == CFG_L && emu_bf16x6();
    if (l.g.pmode && l.g.splits == 1) {  // post_ok: FAST 128x128 (the post-op in the epilogue)
      if (emu) {
        prof_kernel("void rgan::gemm_post_bf16x6<%d>(rgan::GemmArgs)", MODE);
        gemm_post_bf16x6<MODE><<<l.grid, 256, 0, l.s>>>(l.g);
      } else {
        prof_kernel("void rgan::gemm_post<%d>(rgan::GemmArgs)", MODE);
        gemm_post<MODE><<<l.grid, 256, 0, l.s>>>(l.g);
      }
      return;
    }
    if (emu) {
      prof_kernel("void rgan::gemm_bf16x6<%d>(rgan::GemmArgs)", MODE);
      gemm_bf16x6<MODE><<<l.grid, 256, 0, l.s>>>(l.g);
      return;
    }
  }
  switch (l.cfg) {
    case CFG_L: launch_cfg<MODE, 128, 128, 2, 2>(l); break;
    case CFG_M: launch_cfg<MODE, 128, 64, 2, 2>(l); break;
    case CFG_S: launch_cfg<MODE, 64, 64, 2, 2>(l); break;
    default: launch_cfg<MODE, 256, 32, 4, 1>(l); break;
  }
}

}  // namespace rgan
