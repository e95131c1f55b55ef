// run_plan -- a Plan (conv_plan.hip) turned into launches -- and the convolution entry points of the
// C ABI.  The kernels and their launchers are in gemm_conv.hip / gemm_convt2.hip / gemm_wgrad.hip
// (the implicit GEMM of gemm_body.h), conv_reduce.hip, conv_narrow.hip and conv_pack.hip; the launch
// profiler is conv_prof.hip.
#include "conv_plan.h"

namespace rgan {

static int run_plan(Plan& p, void* ws, size_t ws_bytes, hipStream_t s) {
  if (ws_bytes < plan_ws_bytes(p)) return RGAN_EINVAL;
  if (p.mode == MODE_NARROW_T || p.mode == MODE_NARROW_IN || p.mode == MODE_DENSE1 || p.mode == MODE_NARROW3 ||
      p.mode == MODE_NARROW3W) {
    const float* packed = p.prepacked;
    if (p.pack && !packed) {
      if (!ws) return RGAN_EINVAL;
      launch_pack_plan(p, (float*)ws, s);
      RGAN_CHECK_LAUNCH();
      packed = (const float*)ws;
    }
    if (p.slab_floats)  // narrow ConvT channel-split partial sums, after the pack
      p.na.slab = (float*)((char*)ws + (p.prepacked ? 0 : align_up(p.pack_floats * 4, 256)));
    return timed_launch(s, [&]() -> int {
      if (p.mode == MODE_DENSE1) return run_dense1(p, packed, s);
      if (p.mode == MODE_NARROW3 || p.mode == MODE_NARROW3W) return run_narrow3(p, s);
      return run_narrow(p, packed, s);
    });
  }
  if (p.g.M <= 0 || p.g.N <= 0 || p.g.K <= 0) return RGAN_EINVAL;
  char* w = (char*)ws;
  if (p.pack && p.prepacked) {
    p.g.Bw = p.prepacked;
  } else if (p.pack) {
    if (!ws) return RGAN_EINVAL;
    p.pk.out = (float*)w;
    p.g.Bw = p.pk.out;
    w += align_up(p.pack_floats * 4, 256);
    launch_pack(p.pk, s);
    RGAN_CHECK_LAUNCH();
  }
  p.g.slab = p.slab_floats ? (float*)w : nullptr;
  float* tap_dst = nullptr;
  long long tap_osb = 0;
  if (p.tap_stage && !aligned16(p.g.C)) p.tap_stage = false;  // workspace stays sized for it
  const int accum = p.g.accum;
  if (p.tap_stage) {
    tap_dst = p.g.C;
    tap_osb = p.g.out.sb;
    p.g.accum = 0;  // the staging buffer is written fresh; taps_transpose accumulates
    p.g.C = (float*)(w + align_up(p.slab_floats * 4, 256));
    p.g.out = make_out(1, 1, 1, p.g.N, 0, 0, 1, p.g.N, 0, 0, 1);  // [M][N], n contiguous
  }
  p.g.vec_out = vec_out(p, true);
  p.bn_fused = p.bn_part && (bn_epilogue_ok(p) || bn_reduce_ok(p, true));
  p.g.bnp = p.bn_fused ? p.bn_part : nullptr;
  p.post_fused = p.post && !p.bn_fused && post_ok(p, p.post->mode, p.post->nseg, true) &&
                 (p.post->mode != 2 || bn_epilogue_segments(p) <= p.post->part_segments);
  if (p.post_fused) {
    const RganPost& q = *p.post;
    p.g.pmode = q.mode; p.g.pact = q.act; p.g.palpha = q.alpha; p.g.pnseg = q.nseg;
    p.g.px = q.x; p.g.pst = q.stats; p.g.pgam = q.gamma; p.g.pbet = q.beta; p.g.ppart = q.part;
  } else {
    p.g.pmode = 0;
  }
  int bm, bn;
  tile_dims(p.cfg, bm, bn);
  const int tiles_m = ceil_div(p.g.M, bm);
  p.g.nph = p.phases;
  p.g.xgroup = p.fast && p.mode != MODE_WGRAD && tiles_m % 8 == 0 ? 3 : 0;
  // weight-column grouping where the weights dominate: under A-row grouping every XCD fetches
  // the whole weight (D's 2048 -> 4096 conv at C3: 4.36 GB of FETCH per launch for a 537 MB
  // weight; 1.01 GB grouped by weight columns).  Under weight-column grouping every XCD reads
  // the input through its im2col windows instead, which costs more than the input's bytes: at
  // a 2:1 weight / input ratio (D's 1024 -> 2048 conv) it fetched 2.02 GB against 1.33, hence
  // the factor 4 (run r4g)
  if (p.fast && p.mode != MODE_WGRAD && p.g.tiles_n % 8 == 0 &&
      (long long)p.g.bw_bytes * p.phases > 4LL * p.g.a_bytes && tiles_m * p.phases > 1)
    p.g.xgroup = 2;
  dim3 grid = p.g.xgroup ? dim3(tiles_m * p.g.tiles_n * p.phases, 1, p.g.splits)
                         : dim3(tiles_m * p.g.tiles_n, 1, p.phases * p.g.splits);
  const GemmLaunch l{p.g, p.cfg, p.av, p.bv, p.fast, grid, s};
  const int rc = timed_launch(s, [&]() -> int {
    switch (p.mode) {
      case MODE_CONV: launch_gemm_conv(l); break;
      case MODE_CONVT2: launch_gemm_convt2(l); break;
      default: launch_gemm_wgrad(l); break;
    }
    return 0;
  });
  if (rc) return rc;
  p.g.accum = accum;
  if (p.tap_stage) {
    launch_taps_transpose(p.g.C, tap_dst, p.g.M, p.g.N / 16, tap_osb, p.g.accum, s);
    RGAN_CHECK_LAUNCH();
  }
  return p.g.splits > 1 ? launch_splitk_reduce(p, s) : 0;
}

}  // namespace rgan

using namespace rgan;

extern "C" size_t rgan_conv_workspace(const RganConv* d, int which, int prepacked) {
  Plan p;
  if (plan_placeholder(d, which == 0 || which == 1 ? which : 2, nullptr, p)) return 0;
  if (prepacked && which != 2) p.prepacked = PLACEHOLDER;
  size_t extra = 0;
  if (which == 2)  // bias-gradient reduction scratch (rgan_channel_sum, or the fused per-split sums), after the plan's
    extra = align_up(std::max(rgan_bn_partial_bytes((long long)d->batch * d->hout * d->wout, d->cout),
                              (size_t)p.g.splits * p.g.M * sizeof(double) + 256), 256);
  return align_up(plan_ws_bytes(p), 256) + extra + 256;  // never 0 for a valid descriptor
}


static double conv_flops(const RganConv* d) {
  if (!d) return 0.0;  // (the planner refuses it next)
  const double pix = d->transposed ? (double)d->hin * d->win : (double)d->hout * d->wout;
  return 2.0 * d->batch * (double)d->cin * d->cout * d->kh * d->kw * pix;
}

extern "C" int rgan_conv_fwd(const RganConv* d, const float* x, const float* w, const float* wpacked,
                             const float* wscale, const float* bias, float* y, int act, float act_alpha, void* ws,
                             size_t ws_bytes, void* stream) {
  RGAN_REQUIRE(act_ok(act));
  if (!x || (!w && !wpacked) || !y) return RGAN_EINVAL;
  prof_set_flops(conv_flops(d));
  Plan p;
  int rc = plan_fwd(d, x, w, wscale, bias, y, act, act_alpha, p);
  if (rc) return rc;
  if (!p.pack && !w) return RGAN_EINVAL;  // kernels that read the torch layout
  p.prepacked = wpacked;
  return run_plan(p, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" long long rgan_conv_bn_segments(const RganConv* d, int segs) {
  Plan p;
  if (segs < 1 || plan_placeholder(d, 0, nullptr, p)) return 0;
  if (p.mode != MODE_CONV && p.mode != MODE_CONVT2) return 0;
  p.g.vec_out = vec_out(p, false);
  p.bn_segs = segs;
  return (bn_epilogue_ok(p) || bn_reduce_ok(p, false)) ? bn_epilogue_segments(p) : 0;
}

extern "C" int rgan_conv_fwd_bn(const RganConv* d, const float* x, const float* w, const float* wpacked,
                                const float* wscale, const float* bias, float* y, void* ws, size_t ws_bytes,
                                double* bn_part, long long part_segments, int segs, int* fused, void* stream) {
  if (!x || (!w && !wpacked) || !y || !fused || segs < 1) return RGAN_EINVAL;
  *fused = 0;
  prof_set_flops(conv_flops(d));
  Plan p;
  int rc = plan_fwd(d, x, w, wscale, bias, y, 0, 0.f, p);
  if (rc) return rc;
  if (!p.pack && !w) return RGAN_EINVAL;
  p.prepacked = wpacked;
  const bool want = bn_part && p.mode != MODE_NARROW_T && p.mode != MODE_NARROW_IN && p.mode != MODE_DENSE1 &&
                    bn_epilogue_segments(p) <= part_segments;
  p.bn_part = want ? bn_part : nullptr;
  p.bn_segs = segs;
  rc = run_plan(p, ws, ws_bytes, (hipStream_t)stream);
  if (rc) return rc;
  *fused = p.bn_fused ? 1 : 0;
  return 0;
}

extern "C" int rgan_conv_dgrad(const RganConv* d, const float* dy, const float* w, const float* wpacked,
                               const float* wscale, float* dx, void* ws, size_t ws_bytes, void* stream) {
  if (!dy || (!w && !wpacked) || !dx) return RGAN_EINVAL;
  prof_set_flops(conv_flops(d));
  Plan p;
  int rc = plan_dgrad(d, dy, w, wscale, dx, p);
  if (rc) return rc;
  if (!p.pack && !w) return RGAN_EINVAL;  // kernels that read the torch layout
  p.prepacked = wpacked;
  return run_plan(p, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" long long rgan_conv_post_segments(const RganConv* d, int which, int mode, int nseg, int* phases) {
  Plan p;
  const int rc = plan_placeholder(d, which, nullptr, p);
  if (rc || (which != 0 && which != 1) || mode != 2) return 0;
  p.g.vec_out = vec_out(p, false);
  if (phases) *phases = p.phases;
  return post_ok(p, mode, nseg, false) ? bn_epilogue_segments(p) : 0;
}

extern "C" int rgan_conv_post(const RganConv* d, int which, const float* in, const float* w, const float* wpacked,
                              const float* wscale, float* out, void* ws, size_t ws_bytes, const RganPost* post,
                              int* fused, void* stream) {
  if (!in || (!w && !wpacked) || !out || !fused || !post || (which != 0 && which != 1)) return RGAN_EINVAL;
  if (!post->x || (post->mode != 1 && post->mode != 2) || !act_ok(post->act)) return RGAN_EINVAL;
  if (post->mode == 2 && (!post->stats || !post->part || post->nseg < 1)) return RGAN_EINVAL;
  *fused = 0;
  prof_set_flops(conv_flops(d));
  Plan p;
  int rc = which == 0 ? plan_fwd(d, in, w, wscale, nullptr, out, RGAN_ACT_NONE, 0.f, p)
                      : plan_dgrad(d, in, w, wscale, out, p);
  if (rc) return rc;
  if (!p.pack && !w) return RGAN_EINVAL;
  p.prepacked = wpacked;
  p.post = post;
  rc = run_plan(p, ws, ws_bytes, (hipStream_t)stream);
  if (rc) return rc;
  *fused = p.post_fused ? 1 : 0;
  return 0;
}

extern "C" int rgan_conv_wgrad(const RganConv* d, const float* x, const float* dy, float* dw,
                               float* dbias, int accumulate, void* ws, size_t ws_bytes, void* stream) {
  return rgan_conv_wgrad_rows(d, x, dy, dw, dbias, 0, accumulate, ws, ws_bytes, stream);
}

extern "C" int rgan_conv_wgrad_rows(const RganConv* d, const float* x, const float* dy, float* dw, float* dbias,
                                    long long dbias_row0, int accumulate, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !dy || !dw) return RGAN_EINVAL;
  prof_set_flops(conv_flops(d));
  Plan p;
  int rc = plan_wgrad(d, x, dy, dw, p);
  if (rc) return rc;
  p.g.accum = accumulate ? 1 : 0;
  p.da.accum = p.g.accum;
  const size_t plan_bytes = align_up(plan_ws_bytes(p), 256);
  // per-output-channel sum of dy over pixel rows [dbias_row0, P) (Conv2d and ConvTranspose2d
  // alike: dy has cout channels), checked before anything is launched
  const long long P = (long long)d->batch * d->hout * d->wout;
  long long sp = 0;
  if (dbias) {
    if (dbias_row0 < 0 || dbias_row0 >= P) return RGAN_EINVAL;
    if ((long long)d->hout * d->wout == 1) {
      sp = d->ys[0];
    } else {
      if (d->ys[1] != 1 || d->ys[3] != d->cout || d->ys[2] != (long long)d->wout * d->cout ||
          d->ys[0] != (long long)d->hout * d->wout * d->cout)
        return RGAN_EINVAL;
      sp = d->cout;
    }
    const size_t need = plan_bytes + rgan_bn_partial_bytes(P - dbias_row0, d->cout);
    if (!ws || ws_bytes < need) return RGAN_EINVAL;
  }
  // a FAST Conv2d weight gradient stages dy as its A operand: the GEMM sums the bias
  // gradient from those tiles (GemmArgs::dbias, from the BK-aligned pixel row db_k0 on)
  // instead of a channel-sum pass over dy
  const bool bias_fused = dbias && p.mode == MODE_WGRAD && p.fast && !d->transposed && ws_bytes >= plan_bytes &&
                          dbias_row0 % BK == 0 && dbias_row0 <= (long long)INT32_MAX &&
                          (p.g.splits == 1 || (size_t)p.g.splits * p.g.M * sizeof(double) <= ws_bytes - plan_bytes);
  if (bias_fused) {
    p.g.dbias = dbias;
    p.g.db_accum = accumulate ? 1 : 0;
    p.g.db_k0 = (int)dbias_row0;
    p.g.dbp = p.g.splits > 1 ? reinterpret_cast<double*>((char*)ws + plan_bytes) : nullptr;
  }
  rc = run_plan(p, ws, ws_bytes, (hipStream_t)stream);
  if (rc) return rc;
  if (dbias && !bias_fused)
    return rgan_channel_sum(dy + dbias_row0 * sp, P - dbias_row0, d->cout, sp, d->ys[1], dbias, accumulate,
                            (char*)ws + plan_bytes, stream);
  return 0;
}
