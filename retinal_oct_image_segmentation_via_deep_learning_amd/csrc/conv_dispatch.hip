// Kernel selection for every convolution: one plan per descriptor (common.h, ConvPlan / WgradPlan), made here in priority
// order.  The entry points launch that plan and the host size queries answer from it, so a buffer sized by a query is the
// buffer the launch writes.  Host code only: the kernels and their launchers live in the files named in common.h.
#include "common.h"
#include <stdlib.h>

// OCT_DISABLE_V2=1: the generic kernels only (igemm_kernel, wgrad_kernel); read once per process
static bool v2_enabled() {
  static const bool on = [] { const char* e = getenv("OCT_DISABLE_V2"); return !(e && e[0] == '1'); }();
  return on;
}

// first layer (1 -> F), the depth-rolling 3x3x3 kernel, igemm2 (the eight-wave GEMM takes the transposed convolutions it
// accepts over), the generic kernel
static ConvPlan plan_conv_forward(const OctConvDesc* d) {
  ConvPlan pl = {};
  if (v2_enabled()) {
    if (first_plan(d, &pl) || roll3d_plan(d, &pl)) return pl;
    if (igemm2_plan(d, &pl)) {
      gemm1_plan(d, &pl);
      return pl;
    }
  }
  igemm_plan(d, &pl);
  return pl;
}

// first layer (direct, matrix-pipe, all depth taps), wgrad2 (3x3, 1x1, the row-shifted 7x3 launches), the generic kernel
static WgradPlan plan_conv_wgrad(const OctWgradDesc* d, bool dbias, bool dy_coef) {
  WgradPlan pl = {};
  if (v2_enabled() && (first_wgrad_plan(d, dbias, dy_coef, &pl) || wgrad2_plan(d, &pl))) return pl;
  wgrad_plan(d, &pl);
  return pl;
}

// kernel size of a descriptor: kh = kw = 0 means "from taps" (9 -> 3x3, 1 -> 1x1), as before the fields existed
static bool kernel_size(int taps, int kh_in, int kw_in, int* kh, int* kw) {
  if (kh_in == 0 && kw_in == 0) {
    if (taps == 9) { *kh = 3; *kw = 3; return true; }
    if (taps == 1) { *kh = 1; *kw = 1; return true; }
    return false;
  }
  *kh = kh_in; *kw = kw_in;
  return taps == kh_in * kw_in && ((kh_in == 3 && kw_in == 3) || (kh_in == 1 && kw_in == 1) || (kh_in == 7 && kw_in == 3));
}

extern "C" int oct_conv_stat_blocks(const OctConvDesc* d) { return d ? plan_conv_forward(d).stat_rows : 0; }

extern "C" int oct_conv_forward(const OctConvDesc* d, const OctConvArgs* a, void* stream) {
  OCT_CHECK(d && a, "oct_conv_forward: null descriptor");
  OCT_CHECK(d->dtype == OCT_DT_BF16 || d->dtype == OCT_DT_F32, "oct_conv_forward: bad dtype %d", d->dtype);
  int kh = 0, kw = 0;
  OCT_CHECK(kernel_size(d->taps, d->kh, d->kw, &kh, &kw),
            "oct_conv_forward: kernel must be 3x3 (taps 9), 1x1 (taps 1) or 7x3 (taps 21, kh=7, kw=3); got taps=%d kh=%d kw=%d",
            d->taps, d->kh, d->kw);
  OCT_CHECK(kh != 7 || (d->in_mode == OCT_IN_PLAIN && d->out_mode == OCT_OUT_PLAIN), "oct_conv_forward: 7x3 runs plain -> plain");
  OCT_CHECK(d->depth >= 0 && (d->depth == 0 || (d->n % d->depth) == 0), "oct_conv_forward: n=%d is not a whole number of depth-%d volumes", d->n, d->depth);
  OCT_CHECK(d->depth == 0 || kh != 7, "oct_conv_forward: depth taps go with the 3x3 (3x3x3) and 1x1 (2x2x2 transposed) kernels");
  OCT_CHECK(d->out_img_mul == 0 || d->out_mode == OCT_OUT_D2S, "oct_conv_forward: the output image map belongs to D2S");
  OCT_CHECK(d->n > 0 && d->h > 0 && d->w > 0 && d->c0 > 0 && d->c1 >= 0 && d->cout > 0,
            "oct_conv_forward: bad shape n=%d h=%d w=%d c0=%d c1=%d cout=%d", d->n, d->h, d->w, d->c0, d->c1, d->cout);
  OCT_CHECK(a->x0 && a->wpacked && a->y0, "oct_conv_forward: null tensor");
  OCT_CHECK(d->c1 == 0 || a->x1, "oct_conv_forward: c1 > 0 but x1 is null");
  OCT_CHECK(!(d->in_mode == OCT_IN_S2D && d->c1 != 0), "oct_conv_forward: S2D input takes one source");
  OCT_CHECK(!(d->out_mode == OCT_OUT_D2S && (d->cout & 3)), "oct_conv_forward: D2S needs cout %% 4 == 0");
  OCT_CHECK(d->split >= 0 && d->split < d->cout, "oct_conv_forward: bad split %d", d->split);
  OCT_CHECK(d->split == 0 || a->y1, "oct_conv_forward: split without y1");
  OCT_CHECK(d->xform0 >= 0 && d->xform0 <= OCT_XF_AFFINE && d->xform1 >= 0 && d->xform1 <= OCT_XF_AFFINE, "oct_conv_forward: bad xform");
  OCT_CHECK(!(d->xform0 && (!a->scale0 || !a->shift0)), "oct_conv_forward: xform0 without scale/shift");
  OCT_CHECK(!(d->xform1 && (!a->scale1 || !a->shift1)), "oct_conv_forward: xform1 without scale/shift");
  OCT_CHECK(!(d->want_stats && !a->stat_partials), "oct_conv_forward: want_stats without buffer");
  OCT_CHECK((size_t)d->n * d->h * d->w < (1u << 31), "oct_conv_forward: too many pixels");
  const ConvPlan pl = plan_conv_forward(d);
  hipStream_t s = as_stream(stream);
  switch (pl.path) {
    case CONV_FIRST: return launch_first(pl, d, a, s);
    case CONV_ROLL3D: return launch_roll3d(pl, d, a, s);
    case CONV_GEMM1: return launch_gemm1(pl, d, a, s);
    case CONV_IGEMM2: return launch_igemm2(pl, d, a, s);
    default: return launch_igemm(pl, d, a, s);
  }
}

// Number of partial slabs a launch with this descriptor writes in partials mode (OctWgradDesc.partials = 1): the caller
// sizes dwp as [slabs][taps][cout][ktot] (and dbias_partials as [slabs][cout]) and hands `slabs` to the unpack pass.
extern "C" int oct_conv_wgrad_partials(const OctWgradDesc* d) {
  int kh, kw;
  if (!d || !kernel_size(d->taps, d->kh, d->kw, &kh, &kw)) return 0;
  return plan_conv_wgrad(d, false, false).slabs;
}

// Host query behind OctWgradArgs.dy_coef: whether oct_conv_wgrad can apply the BatchNorm backward on load for this
// descriptor (the first-layer kernels but the 7x3 one; OCT_DISABLE_V2=1 switches it off with the other pipelined kernels,
// and the caller then materialises dY with oct_bn_bwd_apply).
extern "C" int oct_conv_wgrad_fused_apply_ok(const OctWgradDesc* d) {
  return d && d->kh != 7 && plan_conv_wgrad(d, false, false).path == WGRAD_FIRST;
}

// Host query behind OctWgradArgs.dy_coef + dy_out: the wgrad2 launch of this descriptor can apply the BatchNorm backward on
// load and store dY for the data gradient (wgrad2_apply_store_ok holds the conditions, next to the kernel they describe)
extern "C" int oct_conv_wgrad_apply_store_ok(const OctWgradDesc* d) {
  int kh, kw;
  if (!d || d->dtype != OCT_DT_BF16 || !kernel_size(d->taps, d->kh, d->kw, &kh, &kw)) return 0;
  if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->c0 <= 0 || d->c1 < 0 || d->cout <= 0) return 0;
  return wgrad2_apply_store_ok(d, plan_conv_wgrad(d, false, false)) ? 1 : 0;
}

// Host query: 1 when oct_conv_wgrad accepts in_img_shift = OCT_IMG_SHIFT_ALL for this descriptor (all three depth taps of a
// Conv3d(1 -> F) weight gradient in one launch, dwp = [3][9][cout]); else the caller launches once per depth tap.
extern "C" int oct_conv_wgrad_all_depth_taps_ok(const OctWgradDesc* d) {
  if (!d) return 0;
  const WgradPlan pl = plan_conv_wgrad(d, false, false);
  return pl.path == WGRAD_FIRST && pl.all_depth_taps;
}

extern "C" int oct_conv_wgrad(const OctWgradDesc* d, const OctWgradArgs* a, void* stream) {
  OCT_CHECK(d && a, "oct_conv_wgrad: null descriptor");
  OCT_CHECK(d->dtype == OCT_DT_BF16 || d->dtype == OCT_DT_F32, "oct_conv_wgrad: bad dtype %d", d->dtype);
  int kh = 0, kw = 0;
  OCT_CHECK(kernel_size(d->taps, d->kh, d->kw, &kh, &kw),
            "oct_conv_wgrad: kernel must be 3x3 (taps 9), 1x1 (taps 1) or 7x3 (taps 21, kh=7, kw=3); got taps=%d kh=%d kw=%d",
            d->taps, d->kh, d->kw);
  OCT_CHECK(kh != 7 || (d->dy_mode == OCT_IN_PLAIN && !a->dy_coef), "oct_conv_wgrad: 7x3 takes a plain dY");
  OCT_CHECK(d->depth >= 0 && (d->depth == 0 || ((d->n % d->depth) == 0 && kh != 7)), "oct_conv_wgrad: bad depth %d for n=%d", d->depth, d->n);
  OCT_CHECK(((d->in_img_shift >= -1 && d->in_img_shift <= 1) || d->in_img_shift == OCT_IMG_SHIFT_ALL) && (d->in_img_shift == 0 || d->depth > 0),
            "oct_conv_wgrad: in_img_shift needs depth > 0");
  OCT_CHECK(d->in_img_shift != OCT_IMG_SHIFT_ALL || oct_conv_wgrad_all_depth_taps_ok(d),
            "oct_conv_wgrad: OCT_IMG_SHIFT_ALL is not available for this descriptor (oct_conv_wgrad_all_depth_taps_ok)");
  OCT_CHECK(d->dy_img_mul == 0 || d->dy_mode == OCT_IN_S2D, "oct_conv_wgrad: the dY image map belongs to S2D");
  OCT_CHECK(d->n > 0 && d->h > 0 && d->w > 0 && d->c0 > 0 && d->c1 >= 0 && d->cout > 0, "oct_conv_wgrad: bad shape");
  OCT_CHECK(a->x0 && a->dy && a->dwp, "oct_conv_wgrad: null tensor");
  OCT_CHECK(d->c1 == 0 || a->x1, "oct_conv_wgrad: c1 > 0 but x1 is null");
  OCT_CHECK(!(d->dy_mode == OCT_IN_S2D && (d->cout & 3)), "oct_conv_wgrad: S2D dy needs cout %% 4 == 0");
  OCT_CHECK(d->xform0 >= 0 && d->xform0 <= OCT_XF_AFFINE && d->xform1 >= 0 && d->xform1 <= OCT_XF_AFFINE, "oct_conv_wgrad: bad xform");
  OCT_CHECK(!(d->xform0 && (!a->scale0 || !a->shift0)), "oct_conv_wgrad: xform0 without scale/shift");
  OCT_CHECK(!(d->xform1 && (!a->scale1 || !a->shift1)), "oct_conv_wgrad: xform1 without scale/shift");
  OCT_CHECK(!d->partials || !a->dbias || a->dbias_partials, "oct_conv_wgrad: partials mode with a bias gradient needs dbias_partials");
  // dy_coef with dy_out: the pipelined 3x3 kernel applies the BatchNorm backward on load and stores dY (wgrad2.hip, DYAPPLY)
  const bool apply_store = a->dy_coef && a->dy_out;
  OCT_CHECK(!a->dy_out || a->dy_coef, "oct_conv_wgrad: dy_out goes with dy_coef");
  OCT_CHECK(!apply_store || oct_conv_wgrad_apply_store_ok(d),
            "oct_conv_wgrad: dy_coef + dy_out is not available for this descriptor (oct_conv_wgrad_apply_store_ok)");
  OCT_CHECK(!apply_store || !a->dbias, "oct_conv_wgrad: dy_coef + dy_out takes no bias gradient");
  const WgradPlan pl = plan_conv_wgrad(d, a->dbias != nullptr, a->dy_coef != nullptr && !apply_store);
  OCT_CHECK(!a->dy_coef || apply_store || pl.path == WGRAD_FIRST, "oct_conv_wgrad: the fused BN-backward apply is only implemented for the 1->F first layer in bf16");
  OCT_CHECK(!a->dy_coef || (a->dy_y && a->dy_scale && a->dy_shift), "oct_conv_wgrad: fused apply needs y, scale, shift");
  if (d->partials) {   // the caller sized dwp from oct_conv_wgrad_partials, which plans without the launch's arguments
    const int slabs = plan_conv_wgrad(d, false, false).slabs;
    OCT_CHECK(pl.slabs == slabs, "oct_conv_wgrad: with these arguments the launch writes %d partial slabs, oct_conv_wgrad_partials "
              "answered %d (first layer with a bias gradient?)", pl.slabs, slabs);
  }
  hipStream_t s = as_stream(stream);
  switch (pl.path) {
    case WGRAD_FIRST: return launch_first_wgrad(pl, d, a, s);
    case WGRAD_W2: return launch_wgrad2(pl, d, a, s);
    default: return launch_wgrad(pl, d, a, s);
  }
}

// Fused backward of a 32 -> 32 layer (igemm2.hip, FUSE): the library decides, the caller asks.  OCT_DISABLE_V2=1 switches it
// off with the other pipelined kernels.
static bool plan_conv_backward_fused(const OctWgradDesc* d, ConvPlan* pl) {
  return d && v2_enabled() && igemm2_fused_plan(d, pl);
}

extern "C" int oct_conv_backward_fused_ok(const OctWgradDesc* d) {
  ConvPlan pl;
  return plan_conv_backward_fused(d, &pl) ? 1 : 0;
}

extern "C" int oct_conv_backward_fused_blocks(const OctWgradDesc* d) {
  ConvPlan pl;
  return plan_conv_backward_fused(d, &pl) ? pl.stat_rows : 0;
}

extern "C" int oct_conv_backward_fused(const OctWgradDesc* d, const OctConvBwdFusedArgs* a, void* stream) {
  OCT_CHECK(d && a, "oct_conv_backward_fused: null descriptor");
  ConvPlan pl;
  OCT_CHECK(plan_conv_backward_fused(d, &pl),
            "oct_conv_backward_fused: not available for this descriptor (oct_conv_backward_fused_ok): bf16, 2-D, 3x3, c0 = cout = 32, "
            "c1 = 0, BN + ReLU on load, w %% 32 == 0, h %% 8 == 0, atomics mode");
  OCT_CHECK(a->x && a->scale && a->shift && a->mean && a->invstd && a->dy && a->wpacked && a->dx && a->dwp && a->partials,
            "oct_conv_backward_fused: null tensor");
  return launch_igemm2_fused(pl, d, a, as_stream(stream));
}
