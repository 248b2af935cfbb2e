/*
 * oct_hip.h -- C ABI of liboct_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * U-Net training hot path of ZhangHH233/Retinal_OCT_Image_Segmentation_via_Deep_Learning.
 *
 * The reference has no FFI of its own: its boundary is Python, and every op on
 * the path is a stock torch.nn call.  Each entry point below replaces the torch op(s) at the
 * cited reference call site; INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless marked host.
 *   - the library never allocates or frees memory and never synchronises: work is enqueued on the
 *     hipStream_t passed as `void* stream`; hipSetDevice is the caller's job.
 *   - every function returns 0 on success or a negative code (OCT_E_*); it never throws/aborts.
 *     oct_get_last_error() returns the message of the calling thread's last failure.
 *   - re-entrant: no global mutable state besides the thread-local error string (backward is
 *     called from PyTorch's autograd thread).
 *   - activation tensors are NHWC ("channels-last") in the dtype named by `dtype`
 *     (OCT_DT_BF16 production, OCT_DT_F32 parity mode); accumulation is always fp32.
 *     Parameters, gradients, BN statistics and losses are fp32.  The network input
 *     (B,Cin,H,W) and output (B,Ccls,H,W) keep the reference's NCHW layout.
 */
#ifndef OCT_HIP_H
#define OCT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCT_VERSION 220 /* 0.2.2 (round 3; + oct_seg_loss_*: CE / Dice on network logits, NHWC or NCHW; + oct_seg_loss_*_weighted: class weights, pixel weight map, ignore_index): 7x3 on the pipelined kernels, oct_rowdot_* up to 12 outputs, frozen-BatchNorm backward, depth-rolling 3-D kernel; 0.2.1: + oct_bilinear_resize_*, floor-mode max-pooling (MGU-Net); 0.2.0: (kh,kw) kernels, depth taps, partials, ReLayNet / 3-D / per-class metric entry points */

/* dtypes of activation storage */
#define OCT_DT_BF16 0
#define OCT_DT_F32 1

/* error codes */
#define OCT_OK 0
#define OCT_IMG_SHIFT_ALL 2  /* OctWgradDesc.in_img_shift: all depth taps in one launch */
#define OCT_E_INVALID (-22)  /* bad descriptor / unsupported shape */
#define OCT_E_LAUNCH (-5)    /* hipLaunch failure */
#define OCT_E_NODEVICE (-19) /* no HIP device */

/* source transform applied while a conv stages its input (BN-apply + ReLU fused on load) */
#define OCT_XF_NONE 0
#define OCT_XF_AFFINE_RELU 1 /* a = max(x*scale[c] + shift[c], 0) */
#define OCT_XF_AFFINE 2      /* a = x*scale[c] + shift[c]: a deferred bias add (SD_Layer_Net conv_block.init_conv) */

/* input / output addressing of the implicit GEMM */
#define OCT_IN_PLAIN 0
#define OCT_IN_S2D 1  /* input pixel (y,x) gathers the 2x2 block of a 2H x 2W tensor: k=(dy*2+dx)*C+c */
#define OCT_OUT_PLAIN 0
#define OCT_OUT_D2S 1 /* GEMM column n=(dy*2+dx)*C+co is stored at pixel (2y+dy, 2x+dx), channel co */

/* weight packing modes (fp32 torch layout -> MFMA A-fragment order in the activation dtype) */
#define OCT_PACK_CONV_FPROP 0   /* (Cout,Cin,3,3): row=co,  k=(tap,ci)               */
#define OCT_PACK_CONV_DGRAD 1   /* (Cout,Cin,3,3): row=ci,  k=(flipped tap,co)       */
#define OCT_PACK_DECONV_FPROP 2 /* (Cin,Cout,2,2): row=(dydx,co), k=ci               */
#define OCT_PACK_DECONV_DGRAD 3 /* (Cin,Cout,2,2): row=ci,  k=(dydx,co)              */
#define OCT_PACK_1X1_DGRAD 4    /* (Cout,Cin,1,1): row=ci,  k=co                     */
#define OCT_PACK_1X1_FPROP 5    /* (Cout,Cin,1,1): row=co,  k=ci                     */
/* 3-D (oct_pack_weights3d): Conv3d(3x3x3) and ConvTranspose3d(k=2,s=2) of the cfg5 volumetric U-Net */
#define OCT_PACK_CONV3D_FPROP 6   /* (Cout,Cin,3,3,3): row=co, taps=(kh,kw), k=(kd,ci)                        */
#define OCT_PACK_CONV3D_DGRAD 7   /* (Cout,Cin,3,3,3): row=ci, k=(kd,co), kernel point-reflected in d, h, w   */
#define OCT_PACK_DECONV3D_FPROP 8 /* (Cin,Cout,2,2,2), one depth slice kdi: row=(dydx,co), k=ci              */
#define OCT_PACK_DECONV3D_DGRAD 9 /* (Cin,Cout,2,2,2): row=ci, k=(kd,dydx,co)                                */

const char* oct_version_string(void);
int oct_version(void);
/* copies the calling thread's last error message (NUL terminated) into buf */
int oct_get_last_error(char* buf, size_t len);
/* number of HIP devices visible (0 on a machine without a GPU); never fails */
int oct_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on MFMA (replaces nn.Conv2d(3x3,p=1) YNet_2022.py:578-596 and
 * nn.ConvTranspose2d(k=2,s=2) YNet_2022.py:526-540, forward and data-gradient).
 *   fprop  3x3 : taps=9, IN_PLAIN, OUT_PLAIN, weights packed CONV_FPROP
 *   dgrad  3x3 : taps=9, IN_PLAIN (x0 = dY), OUT_PLAIN (+split for a concat), CONV_DGRAD
 *   deconv fwd : taps=1, IN_PLAIN, OUT_D2S (+bias),  DECONV_FPROP, cout = 4*Cout
 *   deconv dgrd: taps=1, IN_S2D (x0 = dU at 2H x 2W), OUT_PLAIN, DECONV_DGRAD
 * The two sources x0|x1 are a virtual torch.cat((x0,x1),1) (YNet_2022.py:557).
 * ------------------------------------------------------------------------------------------ */
typedef struct OctConvDesc {
  int dtype;         /* OCT_DT_* */
  int n, h, w;       /* batch and GEMM pixel grid (low-res grid for S2D / D2S) */
  int c0, c1;        /* channels of source 0 / 1 (c1 = 0: single source) */
  int cout;          /* GEMM columns (output channels; 4*Cout for D2S) */
  int taps;          /* 9 or 1 */
  int xform0, xform1;
  int in_mode, out_mode;
  int split;         /* OUT_PLAIN: channels [0,split) -> y0, [split,cout) -> y1; 0: all to y0 */
  int want_stats;    /* write per-workgroup partial sum / sum of squares of the fp32 outputs */
  int kh, kw;        /* kernel size; 0, 0 = derive from taps (9 -> 3x3, 1 -> 1x1).  7, 3 with taps = 21 is ReLayNet's
                      * BasicBlock conv (ReLayNet_2017.py:155-160): stride 1, padding ((kh-1)/2, (kw-1)/2), plain in/out */
  int depth;         /* 0: 2-D.  D > 0: the n images are n/D volumes of D slices each (NDHWC) and the GEMM gains depth taps:
                      *   taps 9, plain in : Conv3d 3x3x3, padding 1 -- K = 3*(c0+c1), tap kd reads slice d+kd-1 (zero outside
                      *                      the volume); weights packed OCT_PACK_CONV3D_FPROP / _DGRAD
                      *   taps 1, IN_S2D   : ConvTranspose3d(k2,s2) data gradient -- K = 8*c0, k = (kd,dy,dx,c) gathers from
                      *                      slice 2d+kd of the 2D x 2H x 2W tensor; weights OCT_PACK_DECONV3D_DGRAD        */
  int out_img_mul, out_img_add; /* OUT_D2S only, 0,0 = identity: the output image index is img*mul + add.  ConvTranspose3d
                      * forward = two D2S launches (kd = 0, 1) with mul = 2, add = kd and the OCT_PACK_DECONV3D_FPROP slice */
} OctConvDesc;

typedef struct OctConvArgs {
  const void* x0; const void* x1;
  const float* scale0; const float* shift0; /* per channel of source 0 (xform0 != NONE) */
  const float* scale1; const float* shift1;
  const void* wpacked;                       /* from oct_pack_weights */
  const float* bias;                         /* D2S only, per real output channel; may be NULL */
  void* y0; void* y1;
  float* stat_partials;                      /* [oct_conv_stat_blocks][2][cout] fp32 */
} OctConvArgs;

/* number of partial-statistics rows oct_conv_forward writes (= spatial workgroups) */
int oct_conv_stat_blocks(const OctConvDesc* d);
/* elements (of the activation dtype) of the packed weight buffer for a GEMM with `rows` output
 * rows, `taps` taps and `kch` input channels */
size_t oct_packed_weight_elems(int rows, int taps, int kch);
int oct_pack_weights(int mode, int dtype, const float* w, void* wpacked, int cout, int cin, void* stream);
/* OCT_PACK_CONV_FPROP / OCT_PACK_CONV_DGRAD of a (Cout,Cin,kh,kw) weight with any odd kernel size up to 7x7
 * (buffer: oct_packed_weight_elems(rows, kh*kw, kch)); ReLayNet_2017.py:155-160 uses 7x3.                  */
int oct_pack_weights_kk(int mode, int dtype, const float* w, void* wpacked, int cout, int cin, int kh, int kw,
                        void* stream);
/* The OCT_PACK_*3D modes (buffer: oct_packed_weight_elems(rows, taps, kch) with rows/taps/kch = cout/9/3cin, cin/9/3cout,
 * 4cout/1/cin, cin/1/8cout).  kdi: depth slice for OCT_PACK_DECONV3D_FPROP, 0 otherwise.                         */
int oct_pack_weights3d(int mode, int dtype, const float* w, void* wpacked, int cout, int cin, int kdi, void* stream);
/* The same for up to OCT_PACK_BATCH_MAX weights per launch (all re-packings that follow an optimizer
 * step in one go); longer lists are split.  Jobs are plain structs read on the host.              */
#define OCT_PACK_BATCH_MAX 96
typedef struct OctPackJob {
  int mode, cout, cin, reserved;
  const float* w;   /* torch-layout fp32 weight (device) */
  void* wpacked;    /* oct_packed_weight_elems(...) elements of dtype (device) */
} OctPackJob;
int oct_pack_weights_batch(int dtype, int count, const OctPackJob* jobs, void* stream);
int oct_conv_forward(const OctConvDesc* d, const OctConvArgs* a, void* stream);

/* Weight gradient (replaces the autograd of the same two modules).
 *   3x3   : taps=9, dy plain  -> dwp[tap][cout][ktot]
 *   deconv: taps=1, dy_mode=OCT_IN_S2D (dU at 2H x 2W, cout = 4*Cout) -> dwp[0][(dydx,co)][ci]
 * dwp must be zeroed by the caller; partial sums are accumulated with fp32 atomics.           */
typedef struct OctWgradDesc {
  int dtype;
  int n, h, w;
  int c0, c1;
  int cout;
  int taps;
  int xform0, xform1;
  int dy_mode;
  int kh, kw;        /* as in OctConvDesc; dwp is [kh*kw][cout][ktot] */
  int depth;         /* D > 0: volumes of D slices (see OctConvDesc).  One launch computes the weight gradient of ONE depth
                      * tap: the input tile is read from slice d + in_img_shift (zero outside the volume)              */
  int in_img_shift;  /* -1, 0, +1 = kd - 1 (Conv3d); 0 otherwise; OCT_IMG_SHIFT_ALL: every depth tap in one launch, dwp =
                      * [3][taps][cout][cin] (only where oct_conv_wgrad_all_depth_taps_ok says so)                    */
  int dy_img_mul, dy_img_add; /* dy_mode S2D only, 0,0 = identity: dY is gathered from image img*mul + add
                      * (ConvTranspose3d weight gradient: two launches, mul = 2, add = kd)                               */
  int partials;      /* 0: partial sums of the workgroups meet in dwp through fp32 atomics (dwp zeroed by the caller; the
                      * summation order, hence the last bits, vary from run to run).  1: DETERMINISTIC two-stage reduction --
                      * every workgroup writes its partial sums with plain stores into its own slab of
                      * dwp[oct_conv_wgrad_partials(desc)][taps][cout][ktot] (nothing to zero), and the unpack pass
                      * (OctUnpackJob.nparts) adds the slabs in index order.  Same for the bias gradient through
                      * OctWgradArgs.dbias_partials + oct_reduce_bias_partials.                                          */
} OctWgradDesc;
typedef struct OctWgradArgs {
  const void* x0; const void* x1;
  const float* scale0; const float* shift0;
  const float* scale1; const float* shift1;
  const void* dy;
  float* dwp;
  float* dbias; /* optional: += sum over pixels of dy per real output channel (bias gradient); caller zeroes */
  /* optional fused BatchNorm-backward apply (first layer, or with dy_out below; OCT_E_INVALID elsewhere): when dy_coef != NULL,
   * `dy` holds dA and the kernel forms dy = coef0*[y*scale+shift>0]*dA + coef1*y + coef2 on the fly */
  const void* dy_y; const float* dy_coef; const float* dy_scale; const float* dy_shift;
  float* dbias_partials; /* partials mode with dbias != NULL: [slabs][cout] fp32 (GEMM rows, i.e. 4*Cout for the deconv) */
  /* optional, with dy_coef (where oct_conv_wgrad_apply_store_ok says 1, OCT_E_INVALID elsewhere): the dY the kernel forms is
   * also stored here, [n,h,w,cout] in bf16 -- bit for bit what oct_bn_bwd_apply_to(dy_out, dy, dy_y, dy_coef, dy_scale,
   * dy_shift) writes -- for the data gradient that runs next.  dy_out == dy is allowed.  No dbias in this form. */
  void* dy_out;
} OctWgradArgs;
int oct_conv_wgrad(const OctWgradDesc* d, const OctWgradArgs* a, void* stream);
/* slabs a launch of this descriptor writes when partials = 1 (host query, never fails; >= 1) */
int oct_conv_wgrad_partials(const OctWgradDesc* d);
/* dbias[c] (+)= sum over slabs, in order, of the `rows / channels` GEMM rows that map to channel c (rows = 4*Cout for the
 * transposed convolution, else Cout)                                                                     */
int oct_reduce_bias_partials(const float* part, int nparts, int rows, int channels, float* dbias, int accumulate,
                             void* stream);
/* 1 when oct_conv_wgrad accepts dy_coef (fused BatchNorm-backward apply) for this descriptor, else 0: the
 * caller then materialises dY with oct_bn_bwd_apply first.  Host-only query, never fails.               */
int oct_conv_wgrad_fused_apply_ok(const OctWgradDesc* d);
/* 1 when oct_conv_wgrad accepts dy_coef together with dy_out for this descriptor (the pipelined 3x3 kernel applies the
 * BatchNorm backward when it stages dY and stores dY for the data gradient: no oct_bn_bwd_apply launch, one read of the
 * tensor less): bf16, plain dY, whole tiles (W % 32, H % 8), partials == 0, and a launch grid of a single channel column --
 * Cout = 32 with 64 input channels.  Host-only query, never fails.                                         */
int oct_conv_wgrad_apply_store_ok(const OctWgradDesc* d);
/* 1 when oct_conv_wgrad accepts in_img_shift = OCT_IMG_SHIFT_ALL for this descriptor (nn.Conv3d(1, F, 3) weight gradient,
 * engine3d: all 27 taps in one pass over dY instead of three), else 0.  Host-only query, never fails.    */
int oct_conv_wgrad_all_depth_taps_ok(const OctWgradDesc* d);
/* Fused backward of a 3x3 convolution with 32 input and 32 output channels whose input is x = relu(bn(y1)) of the
 * convolution below (the second convolution of a U-Net block at full resolution, YNet_2022.py:578-600).  ONE launch reads
 * dY once and produces
 *   dx       = the data gradient dA1, bit-identical to oct_conv_forward with OCT_PACK_CONV_DGRAD weights on dY;
 *   dwp      = the weight gradient [9][cout][cin] as oct_conv_wgrad writes it (fp32 atomics, caller zeroes), for
 *              oct_unpack_wgrad_batch;
 *   partials = the BatchNorm-backward sums of the layer below, [oct_conv_backward_fused_blocks][2][cin]: sum of g and of
 *              g * (y1 - mean) * invstd with g = [y1*scale + shift > 0] ? dA1 (as stored) : 0 -- the rows oct_dact_bn_reduce
 *              would write from dx and y1, for oct_bn_bwd_finalize.  One row per workgroup, summed in a fixed order: the
 *              same bits on every run.
 * in place of oct_conv_wgrad + oct_conv_forward + oct_dact_bn_reduce (three of their passes over a tensor fall away).
 * The descriptor is the layer's OctWgradDesc.  oct_conv_backward_fused_ok is 1 only for bf16, 2-D, taps 9, c0 = cout = 32,
 * c1 = 0, xform0 = OCT_XF_AFFINE_RELU, plain dY, w % 32 == 0, h % 8 == 0, partials = 0 and OCT_DISABLE_V2 unset; for every
 * other descriptor it is 0, _blocks is 0, the launch returns OCT_E_INVALID without touching its outputs, and the caller
 * keeps the three separate launches.  Host-only queries, never fail.                                              */
typedef struct OctConvBwdFusedArgs {
  const void* x;                            /* raw input y1 of the layer, NHWC [n,h,w,32] */
  const float* scale; const float* shift;   /* its BN + ReLU transform (xform0) */
  const float* mean; const float* invstd;   /* BatchNorm statistics of the layer below */
  const void* dy;                           /* gradient wrt the layer's output, NHWC [n,h,w,32] */
  const void* wpacked;                      /* the layer's weight, OCT_PACK_CONV_DGRAD */
  void* dx;                                 /* NHWC [n,h,w,32] */
  float* dwp;                               /* [9][32][32] fp32, zeroed by the caller */
  float* partials;                          /* [oct_conv_backward_fused_blocks][2][32] fp32 */
} OctConvBwdFusedArgs;
int oct_conv_backward_fused_ok(const OctWgradDesc* d);
int oct_conv_backward_fused_blocks(const OctWgradDesc* d);
int oct_conv_backward_fused(const OctWgradDesc* d, const OctConvBwdFusedArgs* a, void* stream);
/* dwp -> torch-layout gradient.  mode: OCT_PACK_CONV_FPROP (grad[co][ci][tap]),
 * OCT_PACK_DECONV_FPROP (grad[ci][co][dydx]) or OCT_PACK_1X1_FPROP (grad[co][ci]).
 * accumulate != 0: grad += */
int oct_unpack_wgrad(int mode, const float* dwp, float* grad, int cout, int cin, int accumulate, void* stream);
/* dwp[kh*kw][cout][cin] -> grad (Cout,Cin,kh,kw) for any kernel size */
int oct_unpack_wgrad_kk(const float* dwp, float* grad, int cout, int cin, int kh, int kw, int accumulate, void* stream);
/* 3-D: OCT_PACK_CONV3D_FPROP   dwp[3][9][cout][cin] (three launches, one slab per depth tap) -> grad (Cout,Cin,3,3,3)
 *      OCT_PACK_DECONV3D_FPROP dwp[0][(dydx,co)][ci] of depth slice kdi -> grad (Cin,Cout,2,2,2)[:, :, kdi]          */
int oct_unpack_wgrad3d(int mode, const float* dwp, float* grad, int cout, int cin, int kdi, int accumulate, void* stream);
/* The same for up to OCT_PACK_BATCH_MAX gradients per launch (a whole backward pass).               */
typedef struct OctUnpackJob {
  int mode, cout, cin, accumulate;
  int nparts, reserved; /* slabs to sum in order (partials mode); 0 or 1: dwp is a single accumulated buffer */
  const float* dwp;   /* [taps][rows][kch] fp32 from oct_conv_wgrad (device) */
  float* grad;        /* torch-layout fp32 gradient (device) */
} OctUnpackJob;
int oct_unpack_wgrad_batch(int count, const OctUnpackJob* jobs, void* stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm2d in training mode (nn.BatchNorm2d, YNet_2022.py:586,598; torch defaults eps=1e-5,
 * momentum=0.1, biased var to normalise, unbiased var into running_var).
 * ------------------------------------------------------------------------------------------ */
/* partials [nblocks][2][c] -> mean, invstd, scale=gamma*invstd, shift=beta-mean*scale, and
 * running_mean/var update (skipped when running_mean == NULL).  count = N*H*W.
 * conv_bias (may be NULL): bias of the conv in front of the BN (BioNet_2020.py:45-53, MGUNet_2021.py).
 * The stored y excludes it -- in training mode it cancels in the BN output and its gradient is
 * exactly zero -- so it only enters the running mean here and the eval-mode shift below.         */
int oct_bn_finalize(const float* partials, int nblocks, int c, double count,
                    const float* gamma, const float* beta, float eps, float momentum,
                    float* running_mean, float* running_var,
                    float* mean, float* invstd, float* scale, float* shift, const float* conv_bias,
                    void* stream);
/* eval mode: scale/shift from the running statistics */
int oct_bn_eval_coeffs(int c, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift,
                       const float* conv_bias, void* stream);

/* a = relu(y*scale+shift); p = maxpool2x2(a)  (nn.MaxPool2d(2,2), YNet_2022.py:516-522).  NaN follows torch: relu keeps it
 * and a window that holds one pools to NaN (also a NaN scale / shift).                              */
int oct_bn_relu_pool_fwd(int dtype, const void* y, const float* scale, const float* shift,
                         void* pooled, int n, int h, int w, int c, void* stream);
/* a = relu(y*scale+shift) materialised (not used on the training path; for tests / export) */
int oct_bn_relu_fwd(int dtype, const void* y, const float* scale, const float* shift,
                    void* out, size_t npix, int c, void* stream);

/* g = (da + route(dpool)) * [y*scale+shift > 0], written to g; partial sums of g and
 * g*xhat (xhat = (y-mean)*invstd) per workgroup into partials[nblocks][2][c].
 * da or dpool may be NULL (not both).  dpool is at (h/2, w/2); the gradient goes to the first
 * maximum of each 2x2 window (ATen max_pool2d tie rule).  g may alias da; without dpool g may be
 * NULL (reduce only: no masked copy is written, oct_bn_bwd_apply re-derives the mask).           */
int oct_dact_bn_reduce(int dtype, const void* da, const void* dpool, const void* y,
                       const float* scale, const float* shift, const float* mean,
                       const float* invstd, void* g, float* partials, int n, int h, int w, int c,
                       void* stream);
int oct_dact_bn_reduce_blocks(int n, int h, int w, int c, int has_pool);
/* Pooled layers (nn.MaxPool2d(2, 2) behind conv + BN + ReLU, YNet_2022.py:516-522) without a stored masked gradient: when
 * oct_bn_bwd_apply_pool_ok(...) == 1, oct_dact_bn_reduce(da, dpool, ..., g = NULL) is the reduce-only pass and
 * oct_bn_bwd_apply_pool re-derives g (pool routing to the first maximum + ReLU mask, rounded to the activation dtype) and
 * writes dy = coef0*g + coef1*y + coef2 -- bit-identical to reduce(g) + oct_bn_bwd_apply(g), 11 instead of 12.5 bytes per
 * element.  da may be NULL (no skip gradient); dy may alias da.                                              */
int oct_bn_bwd_apply_pool_ok(int dtype, int n, int h, int w, int c);
int oct_bn_bwd_apply_pool(int dtype, const void* da, const void* dpool, const void* y, const float* scale,
                          const float* shift, const float* coef, void* dy, int n, int h, int w, int c, void* stream);
/* partials -> dgamma, dbeta and the three coefficients of dy = k[0]*g + k[1]*y + k[2]        */
int oct_bn_bwd_finalize(const float* partials, int nblocks, int c, double count,
                        const float* gamma, const float* mean, const float* invstd,
                        float* dgamma, float* dbeta, float* coef /* [3][c] */, int accumulate,
                        void* stream);
/* dy = coef0*g + coef1*y + coef2, in place over g.  With scale/shift != NULL, g holds dA and the ReLU
 * mask [y*scale+shift > 0] is applied here (pairs with oct_dact_bn_reduce(g = NULL), reduce-only). */
int oct_bn_bwd_apply(int dtype, void* g, const void* y, const float* coef, const float* scale,
                     const float* shift, size_t npix, int c, void* stream);
/* The same, written to `dst` (g is left intact: a gradient that autograd still hands to another consumer -- the
 * residual branch of SD_Layer_Net's conv_block, common.py:22-25 -- needs no copy first). dst == g is allowed.   */
int oct_bn_bwd_apply_to(int dtype, void* dst, const void* g, const void* y, const float* coef, const float* scale,
                        const float* shift, size_t npix, int c, void* stream);
/* ------------------------------------------------------------------------------------------
 * 1x1 convolution with k <= 12 output channels: Attention_block's psi = Conv2d(F_int, 1, 1) (SD_Layer_Net/common.py:79-83)
 * and the heads Conv_1x1 = Conv2d(64, output_ch, 1) (SD_Layer_Net/unet.py:38,113).  Three streaming kernels instead of
 * GEMMs padded k -> 32 (c = 8 * 2^j <= 512 with k <= 4, c <= 128 with k = 5..12 -- ReLayNet's / MGU-Net's class heads: oct_rowdot_ok; other shapes stay on oct_conv_forward / oct_conv_wgrad).
 * x, dx: [npix][c] NHWC; y, dy: [npix][k]; w, dw: [k][c] fp32 (torch (k,c,1,1)).
 *   fwd       : y = x . w^T; stats (may be NULL): [oct_rowdot_blocks][2][k] partial sum / sum of squares (oct_bn_finalize rows)
 *   bwd_data  : dx[pix][c] = sum_k dy[pix][k] * w[k][c]
 *   bwd_weight: dw[k][c] (+)= sum_pix dy[pix][k] * x[pix][c]; partials: scratch [oct_rowdot_blocks][k*c], summed in a fixed order
 * ------------------------------------------------------------------------------------------ */
int oct_rowdot_ok(int c, int k);
int oct_rowdot_blocks(size_t npix, int c);
int oct_rowdot_fwd(int dtype, const void* x, const float* w, void* y, float* stats, size_t npix, int c, int k, void* stream);
int oct_rowdot_bwd_data(int dtype, const void* dy, const float* w, void* dx, size_t npix, int c, int k, void* stream);
int oct_rowdot_bwd_weight(int dtype, const void* dy, const void* x, float* dw, float* partials, size_t npix, int c, int k,
                          int accumulate, void* stream);
/* + the bias gradient dbias[k] (+)= sum_pix dy[pix][k] from the same pass (library 0.2.2); partials: [oct_rowdot_blocks][k*c + k] */
int oct_rowdot_bwd_weight_bias(int dtype, const void* dy, const void* x, float* dw, float* dbias, float* partials, size_t npix, int c,
                               int k, int accumulate, void* stream);

/* per-channel sum over pixels of an NHWC tensor (bias gradient of ConvTranspose2d) */
int oct_channel_sum(int dtype, const void* x, float* out, size_t npix, int c, int accumulate,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * Head: 1x1 conv + Softmax2d (YNet_2022.py:543-546,569) fused with the loss head the reference
 * lacks: CE = nll_loss(log p) and soft Dice.
 * ------------------------------------------------------------------------------------------ */
typedef struct OctHeadDesc {
  int dtype;
  int n, h, w;
  int feat;      /* input channels of the 1x1 conv (init_features) */
  int classes;   /* <= OCT_MAX_CLASSES */
} OctHeadDesc;
#define OCT_MAX_CLASSES 16
#define OCT_HEAD_LOSS_SLOTS (2 + 3 * OCT_MAX_CLASSES)
int oct_head_blocks(const OctHeadDesc* d);
/* forward: y (NHWC dtype) -> probs (NCHW fp32, may be NULL), argmax (int64 [n,h,w], may be NULL);
 * when target != NULL also per-workgroup loss partials [blocks][OCT_HEAD_LOSS_SLOTS].         */
int oct_head_forward(const OctHeadDesc* d, const void* y, const float* scale, const float* shift,
                     const float* w /* [classes][feat] */, const float* b, const int64_t* target,
                     float* probs, int64_t* argmax, float* logits /* NCHW fp32, may be NULL */,
                     double* loss_partials, void* stream);
/* reduces the partials: loss_out[0..2] = total, ce, dice; dice_coef[2][classes] for backward  */
int oct_head_loss_finalize(const OctHeadDesc* d, const double* loss_partials, int nblocks,
                           float w_ce, float w_dice, float dice_eps, float* loss_out,
                           float* dice_coef, void* stream);
/* d(loss)/d(logits) as an NHWC tensor of the activation dtype [n,h,w,classes]: recomputes the
 * logits and the softmax from y, then either dl = w_ce*(p - onehot)/N + p*(dp - <p,dp>) with the
 * Dice term dp_c = A_c*onehot_c + B_c taken from dice_coef (fused loss path; dice_coef may be
 * NULL), or dl = p*(dprobs - <p,dprobs>) for an explicit dprobs (NCHW fp32, autograd path).
 * The rest of the head backward is the generic 1x1 machinery: oct_conv_forward (taps=1, weights
 * packed OCT_PACK_1X1_DGRAD) gives dA, oct_conv_wgrad (taps=1) gives dW, oct_channel_sum db.  */
int oct_head_dlogits(const OctHeadDesc* d, const void* y, const float* scale, const float* shift,
                     const float* w, const float* b, const int64_t* target, const float* dice_coef,
                     float w_ce, const float* dprobs, void* dlogits, void* stream);

/* Fused head backward (feat == 32 only, else OCT_E_INVALID -> use the pieces above): in one pass over
 * y it writes dlogits (optional, NHWC dtype; needed by oct_conv_wgrad for dW), dA = W^T dlogits
 * (NHWC dtype, [n,h,w,feat], UNMASKED: pair it with oct_bn_bwd_apply(scale, shift)), the BN-backward
 * partial sums of the masked gradient [oct_head_blocks][2][feat], the bias gradient (atomics into
 * dbias[classes]; caller zeroes) and -- when dweight is not NULL (classes <= 8) -- the weight gradient
 * dW[c][f] = sum dlogits[c]*relu(bn(y))[f] (atomics into dweight[classes][feat], torch layout
 * (Cout,Cin,1,1); caller zeroes), in which case dlogits may be NULL and is then never written.
 * loss_partials (needs target; may be NULL): [oct_head_blocks][OCT_HEAD_LOSS_SLOTS] rows like
 * oct_head_forward's with only the cross-entropy slot filled -- a training step whose loss has no
 * Dice term can skip the forward head pass and feed these rows to oct_head_loss_finalize.
 * bf16 with classes <= 8, a target, dweight and no dlogits runs on the matrix pipe (head_mfma.hip);
 * every other combination on the vector kernel (head.hip).  OCT_HEAD_MFMA=0 forces the latter.     */
int oct_head_backward_fused(const OctHeadDesc* d, const void* y, const float* scale, const float* shift,
                            const float* mean, const float* invstd, const float* w, const float* b,
                            const int64_t* target, const float* dice_coef, float w_ce,
                            const float* dprobs, void* dlogits, void* da, float* partials,
                            float* dbias, float* dweight, double* loss_partials, void* stream);
/* The matrix-pipe head backward without the dA round trip.  dA = W^T dlogits is a function of the <= 8 bf16 numbers
 * dlogits[pixel][*], so the head can hand those 16 B per pixel to the BatchNorm backward of the layer below instead of
 * the 64-B dA row, and the apply pass recomputes dA (same code, same bits) while it reads y.
 *   oct_head_backward_dl_ok : 1 exactly where oct_head_backward_fused runs on the matrix pipe: bf16, feat 32,
 *                             classes <= 8, OCT_HEAD_MFMA not 0.
 *   oct_head_backward_dl    : oct_head_backward_fused (labels, fused dweight -- both required) with dl8 in place of da:
 *                             dl8 [npix][8] in bf16, slots >= classes zero.  partials, dbias, dweight and
 *                             loss_partials as there (same grid, oct_head_blocks; the partial rows are bit-identical).
 *   oct_head_bwd_apply      : dy = coef0*([y*scale+shift > 0] ? bf16(W^T dl) : 0) + coef1*y + coef2, [npix][32] in bf16.
 * oct_head_backward_dl + oct_head_bwd_apply give the bits of oct_head_backward_fused(da) + oct_bn_bwd_apply(da, y, coef,
 * scale, shift).  Not eligible -> OCT_E_INVALID, nothing written.                                                      */
int oct_head_backward_dl_ok(const OctHeadDesc* d);
int oct_head_backward_dl(const OctHeadDesc* d, const void* y, const float* scale, const float* shift,
                         const float* mean, const float* invstd, const float* w, const float* b,
                         const int64_t* target, const float* dice_coef, float w_ce, void* dl8, float* partials,
                         float* dbias, float* dweight, double* loss_partials, void* stream);
int oct_head_bwd_apply(const OctHeadDesc* d, const void* dl8, const void* y, const float* scale, const float* shift,
                       const float* w, const float* coef /* [3][32] */, void* dy, void* stream);

/* ------------------------------------------------------------------------------------------
 * Segmentation loss on logits a network has already produced (U_Net / AttU_Net / AttU_Net4,
 * MGUNet / MGUNet_2, ReLayNet: the networks without the fused head above).  Same loss as the
 * head's -- CE = mean over pixels of -log softmax[target], Dice = 1 - mean_c (2 I_c + eps) /
 * (P_c + Y_c + eps) -- and the same partial rows, so oct_head_loss_finalize reduces them
 * (descriptor: feat = 1).  d->dtype / n / h / w / classes describe the logits; d->feat is not
 * read here.  No atomics: per-lane, wave, workgroup sums, one fp64 row per workgroup.
 *   layout OCT_SEG_NHWC: logits [n,h,w,classes] in d->dtype (the networks' own output)
 *   layout OCT_SEG_NCHW: logits [n,classes,h,w] fp32 (what a network's forward returns)
 * A target outside [0, classes) makes the loss NaN (no check, no synchronisation).
 * ------------------------------------------------------------------------------------------ */
#define OCT_SEG_NHWC 0
#define OCT_SEG_NCHW 1
/* rows of loss_partials the two launches below write (0 for npix == 0 or classes out of [1,16]) */
int oct_seg_loss_blocks(size_t npix, int classes);
/* argmax (int64 [n,h,w], may be NULL): first maximum of the logits wins, as in torch.argmax;
 * loss_partials (may be NULL, needs target): [oct_seg_loss_blocks][OCT_HEAD_LOSS_SLOTS].
 * target == NULL with argmax only is a pure predict.                                            */
int oct_seg_loss_forward(const OctHeadDesc* d, int layout, const void* logits, const int64_t* target,
                         int64_t* argmax, double* loss_partials, void* stream);
/* dlogits (same layout and dtype as the logits) = g * [w_ce (p - onehot)/N + p (dp - <p,dp>)]
 * with dp_c = A_c onehot_c + B_c from oct_head_loss_finalize's dice_coef (NULL: no Dice term)
 * and g = *dloss (device float, NULL: 1).  loss_partials (only with dice_coef == NULL, may be
 * NULL): the cross-entropy rows as well -- slot 0 filled, the Dice slots zero -- so a CE-only
 * training step reads the logits once and feeds these rows to oct_head_loss_finalize.          */
int oct_seg_loss_backward(const OctHeadDesc* d, int layout, const void* logits, const int64_t* target,
                          const float* dice_coef, float w_ce, const float* dloss, void* dlogits,
                          double* loss_partials, void* stream);

/* Weighted forms of the loss above (library 0.2.2, same OCT_VERSION): class weights, a per-pixel
 * weight map and ignore_index, each optional.
 *   class_weight  float [classes] on the device, NULL: 1
 *   pixel_weight  float [n,h,w] on the device, NULL: 1 (a constant of the loss: no gradient)
 *   has_ignore / ignore_index   a pixel whose label equals ignore_index does not count at all
 *   omega_i = [t_i != ignore_index] * class_weight[t_i] * pixel_weight[i]
 *   CE   = sum_i omega_i * (-log softmax[t_i]) / sum_i omega_i
 *          (F.cross_entropy(weight=, ignore_index=) when there is no map)
 *   Dice = over the pixels that are not ignored, otherwise as above and unweighted
 * A label outside [0, classes) that is not the ignored one still gives a NaN loss; sum omega = 0
 * (everything ignored) gives a NaN loss as torch does.  An ignored pixel gets a gradient of
 * exactly 0 in every class.  sum omega never passes through the host: it is reduced on the device
 * (oct_seg_loss_weight_sum, or slot 1 of the forward rows -> oct_seg_loss_finalize_weighted's
 * wsum_out) and oct_seg_loss_backward_weighted reads it there.  No atomics, fixed order.
 *   CE only:   weight_sum -> backward_weighted(loss_partials = rows) -> finalize_weighted
 *   with Dice: forward_weighted -> finalize_weighted(wsum_out) -> backward_weighted(dice_coef)  */
/* sum omega from the labels and the map alone; partials: [oct_seg_loss_blocks] doubles of scratch,
 * wsum: one double.  d->dtype / layout are not read beyond the usual descriptor checks.          */
int oct_seg_loss_weight_sum(const OctHeadDesc* d, const int64_t* target, const float* class_weight,
                            const float* pixel_weight, int has_ignore, int64_t ignore_index,
                            double* partials, double* wsum, void* stream);
/* rows [oct_seg_loss_blocks][OCT_HEAD_LOSS_SLOTS]: slot 0 = sum omega*ce, slot 1 = sum omega, then
 * the Dice sums over the pixels that are not ignored                                             */
int oct_seg_loss_forward_weighted(const OctHeadDesc* d, int layout, const void* logits,
                                  const int64_t* target, const float* class_weight,
                                  const float* pixel_weight, int has_ignore, int64_t ignore_index,
                                  double* loss_partials, void* stream);
/* dlogits = g * valid * [w_ce (p - onehot) omega / *wsum + p (dp - <p,dp>)]; wsum: device double.
 * loss_partials (only with dice_coef == NULL, may be NULL): rows with slots 0 and 1 filled.      */
int oct_seg_loss_backward_weighted(const OctHeadDesc* d, int layout, const void* logits,
                                   const int64_t* target, const float* class_weight,
                                   const float* pixel_weight, int has_ignore, int64_t ignore_index,
                                   const double* wsum, const float* dice_coef, float w_ce,
                                   const float* dloss, void* dlogits, double* loss_partials,
                                   void* stream);
/* oct_head_loss_finalize with CE = slot 0 / slot 1 instead of slot 0 / N; wsum_out (device double,
 * may be NULL) receives slot 1's total                                                           */
int oct_seg_loss_finalize_weighted(const OctHeadDesc* d, const double* loss_partials, int nblocks,
                                   float w_ce, float w_dice, float dice_eps, float* loss_out,
                                   float* dice_coef, double* wsum_out, void* stream);

/* Binary / multi-label head (library 0.2.2, same OCT_VERSION): `classes` independent sigmoid
 * channels instead of one softmax.  Logits as above (layout, d->dtype); the target is a uint8 mask
 * [n,classes,h,w] (NCHW plane order for BOTH logits layouts) with values 0 / 1.
 *   pos_weight    float [classes] on the device, NULL: 1
 *   pixel_weight  float [n,h,w] on the device, NULL: 1; one value for every channel of a pixel
 *   has_ignore / ignore_value (in [2,255])   an element whose target equals it does not count
 *   omega = valid * pixel_weight
 *   l     = (1 - t) x + (1 + (pos_weight[c] - 1) t) (log1p(exp(-|x|)) + max(-x, 0))
 *           (torch's BCEWithLogitsLoss(pos_weight=))
 *   BCE   = sum omega l / sum omega     over all n*classes*h*w elements
 *   Dice  = 1 - mean_c (2 I_c + eps) / (P_c + Y_c + eps),  I_c = sum sigmoid(x) t, P_c = sum
 *           sigmoid(x), Y_c = sum t over the valid elements of channel c, not weighted
 * A valid target that is neither 0 nor 1 gives a NaN loss; everything ignored gives NaN; an
 * ignored element gets a gradient of exactly 0 whatever its logit is (NaN included).  The rows
 * have the layout of oct_seg_loss_forward_weighted's (slot 0 = sum omega*l, slot 1 = sum omega,
 * then I_c, P_c, Y_c) and oct_seg_loss_finalize_weighted reduces them: [loss, bce, dice], the
 * Dice backward coefficients and sum omega.  No atomics, fixed order.
 *   BCE only:  [weight_sum ->] backward(loss_partials = rows) -> finalize_weighted
 *   with Dice: forward -> finalize_weighted(wsum_out) -> backward(dice_coef)
 * weight_sum is needed only with a map or ignore_value: without both, sum omega is the element
 * count and wsum may be NULL.                                                                    */
/* sum omega from the target and the map alone (target may be NULL without has_ignore);
 * partials: [oct_seg_loss_blocks] doubles of scratch, wsum: one double                          */
int oct_bce_loss_weight_sum(const OctHeadDesc* d, const uint8_t* target, const float* pixel_weight,
                            int has_ignore, int ignore_value, double* partials, double* wsum,
                            void* stream);
/* mask (uint8 [n,classes,h,w], may be NULL) = x >= tau, 0 for a NaN logit; loss_partials (may be
 * NULL, needs target): [oct_seg_loss_blocks][OCT_HEAD_LOSS_SLOTS], the Dice slots zero unless
 * want_dice.  target == NULL with a mask only is a pure predict.                                 */
int oct_bce_loss_forward(const OctHeadDesc* d, int layout, const void* logits, const uint8_t* target,
                         const float* pos_weight, const float* pixel_weight, int has_ignore,
                         int ignore_value, int want_dice, float tau, uint8_t* mask,
                         double* loss_partials, void* stream);
/* dlogits (layout and dtype of the logits) = g * valid * [w_bce (omega / sum omega) (s (1 - t +
 * pos_weight t) - pos_weight t) + s (1 - s) (A_c t + B_c)], s = sigmoid(x), A / B from dice_coef
 * (NULL: no Dice term), g = *dloss (NULL: 1), sum omega = *wsum (device double; NULL, allowed
 * without a map and ignore_value: the element count).  loss_partials (only with dice_coef == NULL,
 * may be NULL): rows with slots 0 and 1 filled.                                                  */
int oct_bce_loss_backward(const OctHeadDesc* d, int layout, const void* logits, const uint8_t* target,
                          const float* pos_weight, const float* pixel_weight, int has_ignore,
                          int ignore_value, const double* wsum, const float* dice_coef, float w_bce,
                          const float* dloss, void* dlogits, double* loss_partials, void* stream);

/* ------------------------------------------------------------------------------------------
 * Layout / dtype helpers and the optimizer
 * ------------------------------------------------------------------------------------------ */
/* (B,C,H,W) fp32 -> (B,H,W,C) dtype */
int oct_nchw_to_nhwc(int dtype, const float* x, void* out, int n, int c, int h, int w, void* stream);
/* (B,H,W,C) dtype -> (B,C,H,W) fp32 (tests / export) */
int oct_nhwc_to_nchw(int dtype, const void* x, float* out, int n, int c, int h, int w, void* stream);
/* torch.optim.SGD (momentum, dampening 0, no nesterov): buf = mu*buf + g (buf = g when
 * first != 0); p -= lr*buf.  grad_scale multiplies g first (1/world_size after all-reduce).  */
int oct_sgd_step(float* p, const float* g, float* buf, size_t n, float lr, float momentum,
                 float weight_decay, float grad_scale, int first, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer layer over flat fp32 buffers (library 0.2.2, same OCT_VERSION): Adam / AdamW, the
 * global gradient norm with its clip coefficient, SGD with a device-side gradient scale.
 * Any n >= 1 and any 4-byte-aligned pointers; 16-byte-aligned buffers take the vector path, with
 * the same bits.  No atomics and no synchronisation; the caller owns all memory.
 *   dev_scale  (may be NULL): device pointer to ONE float that multiplies grad_scale -- out + 1 of
 *              oct_grad_norm, so a clipped step needs no host round trip.
 *   decay_mask (may be NULL): one byte per 64 floats, (n + 63) / 64 bytes; 0 = no weight decay for
 *              the chunk (bit for bit the weight_decay = 0 result), anything else = decay.
 * ------------------------------------------------------------------------------------------ */
/* torch.optim.Adam (decoupled == 0) / AdamW (decoupled != 0), single tensor, no amsgrad:
 *   g' = g * (grad_scale * *dev_scale);  Adam: g' += wd p;  AdamW: p *= 1 - lr wd
 *   m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  p -= step_size * m / (sqrt(v) * inv_sqrt_bc2 + eps)
 * step_size = lr / (1 - b1^t) and inv_sqrt_bc2 = 1 / sqrt(1 - b2^t) come from the host (float64,
 * rounded once), as torch computes them; lr itself is read for the decoupled decay only.
 * All-zero p, g, m, v give an update of exactly 0.  eps <= 0, betas outside [0, 1), negative lr /
 * weight_decay / step_size and inv_sqrt_bc2 < 1 are OCT_E_INVALID.                              */
int oct_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int decoupled, float step_size,
                  float inv_sqrt_bc2, float grad_scale, const float* dev_scale,
                  const uint8_t* decay_mask, void* stream);
/* oct_sgd_step with dev_scale and decay_mask; both NULL: the same bits as oct_sgd_step */
int oct_sgd_step_scaled(float* p, const float* g, float* buf, size_t n, float lr, float momentum,
                        float weight_decay, float grad_scale, int first, const float* dev_scale,
                        const uint8_t* decay_mask, void* stream);
/* fp64 rows of `partials` that oct_grad_norm writes: a function of n alone (0 for n == 0) */
int oct_grad_norm_blocks(size_t n);
/* out[0] = || g * grad_scale ||_2, out[1] = min(1, max_norm / (out[0] + 1e-6)) as
 * torch.nn.utils.clip_grad_norm_ (error_if_nonfinite = False: a NaN in g gives NaN, NaN; an Inf
 * gives Inf, 0).  Two launches: fp64 sums of squares in a fixed order, one row per workgroup into
 * partials [oct_grad_norm_blocks(n)], then one workgroup adds the rows in a fixed order.  Same
 * bits on every call.  max_norm <= 0 is OCT_E_INVALID.                                          */
int oct_grad_norm(const float* g, size_t n, float grad_scale, float max_norm, double* partials,
                  float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Building blocks of the reference's other U-Net families; NHWC tensors
 * of `dtype`, materialised activations.
 * ------------------------------------------------------------------------------------------ */
#define OCT_ACT_NONE 0
#define OCT_ACT_RELU 1
#define OCT_ACT_SIGMOID 2
/* out = act(y*scale[c] + shift[c] (+ res)).  Covers BN+ReLU (MGUNet_2021.py:46-55), conv bias
 * without BN (scale=1, shift=bias; MGUNet_2021.py:57-64, common.py:9), the residual sum
 * `conv(x) + init_conv` + act (common.py:21-25), BN+Sigmoid (common.py:77-81).  res may be NULL. */
int oct_affine_act_fwd(int dtype, const void* y, const float* scale, const float* shift,
                       const void* res, int act, void* out, size_t npix, int c, void* stream);
/* The same with a residual whose bias add was deferred (OCT_XF_AFFINE producer): out = act(scale*y + shift + T(res + res_shift[c])),
 * the sum rounded to the storage type first -- bit-identical to a residual that had been materialised.            */
int oct_affine_res_act_fwd(int dtype, const void* y, const float* scale, const float* shift, const void* res,
                           const float* res_shift, int act, void* out, size_t npix, int c, void* stream);
/* dz = dout * act'(z), from the stored output: relu [out>0], sigmoid out*(1-out). dz may alias dout */
int oct_act_bwd(int dtype, const void* dout, const void* out, int act, void* dz, size_t n, void* stream);
/* nn.MaxPool2d(k) on a materialised activation (SD_Layer_Net/unet.py:85, MGUNet_2021.py:211-217);
 * Output (n, h/k, w/k, c), torch's floor mode: trailing rows / columns that no whole window covers are
 * ignored (MGR_Module's 3x3 / 5x5 pools, MGUNet_2021.py:163,168).  Backward writes all of da: dout to the
 * first maximum of each window in row-major order (ATen's tie rule), zero elsewhere.            */
int oct_maxpool_fwd(int dtype, const void* a, void* out, int n, int h, int w, int c, int k, void* stream);
int oct_maxpool_bwd(int dtype, const void* a, const void* dout, void* da, int n, int h, int w, int c,
                    int k, void* stream);
/* nn.Upsample(scale_factor=f, mode="bilinear", align_corners=True) / nn.UpsamplingBilinear2d
 * (common.py:31, MGUNet_2021.py:79,98): x (n,h,w,c) -> out (n,h*f,w*f,c); backward is the exact
 * transpose (dout at h*f x w*f -> dx at h x w), deterministic (gather, no atomics).             */
int oct_bilinear_up_fwd(int dtype, const void* x, void* out, int n, int h, int w, int c, int factor,
                        void* stream);
int oct_bilinear_up_bwd(int dtype, const void* dout, void* dx, int n, int h, int w, int c, int factor,
                        void* stream);
/* F.interpolate(x, size=(ho, wo), mode="bilinear", align_corners=True) (MGR_Module.forward,
 * MGUNet_2021.py:180,184,188): x (n,h,w,c) -> out (n,ho,wo,c) for any output size; src = dst*(in-1)/(out-1),
 * a one-pixel axis reads pixel 0.  Backward is the exact transpose (gather, deterministic).     */
int oct_bilinear_resize_fwd(int dtype, const void* x, void* out, int n, int h, int w, int c, int ho, int wo,
                            void* stream);
int oct_bilinear_resize_bwd(int dtype, const void* dout, void* dx, int n, int h, int w, int c, int ho, int wo,
                            void* stream);
/* Scatter step of nn.ConvTranspose2d(kernel=s, stride=s) (MGUNet_2021.py:95, s=4): the GEMM output
 * in[n,h,w,(dy*s+dx)*cout+co] goes to out[n,h*s+dy,w*s+dx,co] (+ bias[co], may be NULL);
 * space_to_depth is its inverse, used on dOut before the weight / data gradients.               */
int oct_depth_to_space(int dtype, const void* in, const float* bias, void* out, int n, int h, int w,
                       int cout, int s, void* stream);
int oct_space_to_depth(int dtype, const void* in, void* out, int n, int h, int w, int cout, int s,
                       void* stream);
/* Attention gate product `x * psi` (SD_Layer_Net/common.py:91): out[pix,c] = x[pix,c]*p[pix];
 * backward dx = dout*p, dp[pix] = sum_c dout*x.                                                 */
int oct_gate_fwd(int dtype, const void* x, const void* p, void* out, size_t npix, int c, void* stream);
int oct_gate_bwd(int dtype, const void* dout, const void* x, const void* p, void* dx, void* dp,
                 size_t npix, int c, void* stream);

/* ReLayNet blocks (SOTAS/Lesions_Segment/ReLayNet_2017.py:133-201).
 * BasicBlock :164-168: out = prelu(bn(conv7x3(x))) with nn.PReLU()'s single learnable slope `alpha` (device float[1]):
 *   forward  out = z > 0 ? z : alpha*z,  z = y*scale[c] + shift[c]  (y = raw conv output, scale/shift from oct_bn_finalize)
 *   backward dz = dout * (z > 0 ? 1 : alpha);  dalpha[0] += sum dout*z*[z <= 0]  (caller zeroes dalpha); dz may alias dout */
int oct_affine_prelu_fwd(int dtype, const void* y, const float* scale, const float* shift, const float* alpha,
                         void* out, size_t npix, int c, void* stream);
int oct_affine_prelu_bwd(int dtype, const void* dout, const void* y, const float* scale, const float* shift,
                         const float* alpha, void* dz, float* dalpha, size_t npix, int c, void* stream);
/* The same backward WITHOUT the dz tensor (library 0.2.2): the two BatchNorm-backward passes re-derive dz = dout * (z > 0 ? 1 : alpha)
 * themselves -- oct_dact_bn_reduce_prelu (sums for oct_bn_bwd_finalize, dalpha[0] += ...; partial rows as oct_dact_bn_reduce_blocks
 * (n, h, w, c, 0)) and oct_bn_bwd_apply_prelu_to (dst = k0*dz + k1*y + k2) -- bit-identical to oct_affine_prelu_bwd followed by the
 * plain passes.  oct_prelu_bn_fused_ok: c % 8 == 0 with 256 % (c/8) == 0.                                                  */
int oct_prelu_bn_fused_ok(int dtype, int c);
int oct_dact_bn_reduce_prelu(int dtype, const void* da, const void* y, const float* scale, const float* shift, const float* alpha,
                             const float* mean, const float* invstd, float* partials, float* dalpha, int n, int h, int w, int c,
                             void* stream);
int oct_bn_bwd_apply_prelu_to(int dtype, void* dst, const void* da, const void* y, const float* coef, const float* scale,
                              const float* shift, const float* alpha, size_t npix, int c, void* stream);
/* EncoderBlock :174-179, nn.MaxPool2d(k, k, return_indices=True): out (n,h/k,w/k,c) and idx (same shape, int64) holding
 * torch's index of the winner inside its (n, c) input plane, iy*w + ix; first maximum in row-major window order.      */
int oct_maxpool_idx_fwd(int dtype, const void* a, void* out, int64_t* idx, int n, int h, int w, int c, int k, void* stream);
/* DecoderBlock :185-188, nn.MaxUnpool2d: out[n, idx[n,p,c], c] = v[n,p,c] over a zero-filled (by the caller) out of
 * `plane` = H*W pixels per image (also the backward of the pooling above); the gather is its transpose (unpool
 * backward): v[n,p,c] = x[n, idx[n,p,c], c].  npool = pooled pixels per image.  Out-of-range indices are skipped / 0. */
int oct_index_scatter(int dtype, const void* v, const int64_t* idx, void* out, int n, size_t npool, size_t plane, int c,
                      void* stream);
int oct_index_gather(int dtype, const void* x, const int64_t* idx, void* v, int n, size_t npool, size_t plane, int c,
                     void* stream);
/* The same pair by WINDOW CODE (library 0.2.2; the indices of ReLayNet's encoder -> decoder path never leave the library): code
 * (n,h/k,w/k,c) uint8 = (iy - yo*k)*k + (ix - xo*k) of the winner oct_maxpool_idx_fwd would report.  oct_window_scatter writes the
 * WHOLE (n, hp*k, wp*k, c) output (value at the code, zeros elsewhere: no zero-fill by the caller) = MaxUnpool2d forward and
 * max-pool backward; oct_window_gather = MaxUnpool2d backward.  k <= 15.                                                      */
int oct_maxpool_code_fwd(int dtype, const void* a, void* out, unsigned char* code, int n, int h, int w, int c, int k, void* stream);
int oct_window_scatter(int dtype, const void* v, const unsigned char* code, void* out, int n, int hp, int wp, int c, int k, void* stream);
int oct_window_gather(int dtype, const void* x, const unsigned char* code, void* v, int n, int hp, int wp, int c, int k, void* stream);

/* MaxPool3d(2) of the cfg5 volumetric U-Net = oct_bn_relu_pool_fwd inside every slice, then the pairwise maximum of
 * consecutive slices: p2 (nslab, 2, m) -> out (nslab, m), m contiguous elements per slice ((h/2)*(w/2)*c).  Backward:
 * dout goes to the first slice unless the second is strictly larger (torch's first-maximum rule in (d,h,w) order);
 * the 2-D routing inside the slice is oct_dact_bn_reduce's.                                                   */
int oct_depth_pool_fwd(int dtype, const void* p2, void* out, size_t nslab, size_t m, void* stream);
int oct_depth_pool_bwd(int dtype, const void* p2, const void* dout, void* dp2, size_t nslab, size_t m, void* stream);

/* ------------------------------------------------------------------------------------------
 * Metrics (Metrics/Region_based_metrics.py:3-61, Metrics/ConfusionMatrix_based_metrics.py:4-63)
 * One pass over the two masks; integer inputs are reduced exactly in 64-bit with numpy's
 * same-dtype product semantics, float inputs in fp64.
 *   out_i[6] = { sum(t*p), sum(t), sum(p), sum((1-t)*(1-p)), sum((1-t)*p), sum(t*(1-p)) }
 * elem: 0 u8/bool, 1 i32, 2 i64, 3 f32, 4 f64, 5 i8, 6 i16, 7 u16                                   */
int oct_confusion_counts(const void* y_true, const void* y_pred, int elem, size_t n,
                         int64_t* out_i /* [6] device, zeroed by callee */,
                         double* out_f /* [6] device, zeroed by callee */, void* stream);

/* Per-class variant for CLASS MAPS (integer element types only): out[c][6] holds the same six sums for the
 * one-vs-rest masks (y_true == c), (y_pred == c), c = 0..classes-1 (classes <= 16), all classes in ONE pass --
 * what the reference's functions (Region_based_metrics.py:3-61, ConfusionMatrix_based_metrics.py:4-63) compute
 * when they are called once per class on binarised maps.  Labels outside [0, classes) belong to no class.
 * scratch: 48 x uint64 device words (zeroed by the callee).                                               */
int oct_class_confusion_counts(const void* y_true, const void* y_pred, int elem, size_t n, int classes,
                               int64_t* out /* [classes][6] device */, uint64_t* scratch /* [48] device */,
                               void* stream);

/* Metrics/PixelError_based_metrics.py:3-37: out[0] = sum (double(t) - double(p))^2 (device double)      */
int oct_sqdiff_sum(const void* y_true, const void* y_pred, int elem, size_t n, double* out, void* stream);
/* Metrics/Biomarker_based_metrics.py:3-21: out[0] = sum over columns of |colsum(t) - colsum(p)| for a
 * (rows, cols) view (axis 0 = rows).  unsigned_wrap != 0 reproduces numpy's uint64 wrap-around for
 * unsigned inputs; bool masks pass elem 0 with unsigned_wrap = 0 (numpy sums bool in int64).          */
int oct_column_absdiff_sum(const void* y_true, const void* y_pred, int elem, int unsigned_wrap, size_t rows,
                           size_t cols, double* out, void* stream);

/* Streaming segmentation evaluator (library 0.2.2, same OCT_VERSION): ONE launch per batch ADDS the C x C confusion
 * matrix and the per-layer thickness error of a (target, prediction) pair to a device-resident state; nothing is read
 * back, so a validation loop synchronises once, when it reads the state.
 *   target  class map [images][h][w], uint8 (target_elem 0) or int64 (target_elem 2) -- the element codes above
 *   pred    pred_kind OCT_EVAL_PRED_U8 / _I64: a class map of the same shape;
 *           OCT_EVAL_PRED_NHWC_BF16 / _NHWC_F32: logits [images][h][w][classes]; OCT_EVAL_PRED_NCHW_F32: logits
 *           [images][classes][h][w].  p = arg-max over the channels with the rule of oct_seg_loss_forward's arg-max
 *           (first maximum wins, the first NaN beats everything), so p equals what model.predict writes
 *   state   int64[classes*classes + classes + 4], zeroed ONCE by the caller (hipMemsetAsync), C = classes:
 *           [t*C + p]          cm         pixels with label t predicted as p
 *           [C*C + c]          thick_abs  sum over images b and columns x of |T - P|, T = #{y : valid, t == c},
 *                                         P = #{y : valid, p == c}: the thickness axis is h (np.sum(mask, axis=0) of
 *                                         Biomarker_based_metrics.thickness_difference on an h x w mask)
 *           [C*C + C]          columns    += images * w per call
 *           [C*C + C + 1]      ignored    pixels with has_ignore and t == ignore_index; counted here and nowhere else
 *           [C*C + C + 2]      invalid    pixels not ignored whose t or p lies outside [0, C); here and nowhere else
 *           [C*C + C + 3]      updates    += 1 per call
 * A pixel that is neither ignored nor invalid is "valid".  No label indexes anything before it is range-checked.
 * Any h, w >= 1 and ANY base alignment of target / pred are accepted (the class maps are read element-wise, logits take
 * 16-byte loads only where base and row pitch allow them); images * h * w < 2^31, 1 <= classes <= 16.               */
#define OCT_EVAL_PRED_U8 0
#define OCT_EVAL_PRED_I64 1
#define OCT_EVAL_PRED_NHWC_BF16 2
#define OCT_EVAL_PRED_NHWC_F32 3
#define OCT_EVAL_PRED_NCHW_F32 4
#define OCT_EVAL_STATE_EXTRA 4 /* columns, ignored, invalid, updates */
typedef struct {
  int images, h, w, classes; /* images = product of all leading dims; 1 <= classes <= 16 */
  int target_elem;           /* 0 uint8, 2 int64 */
  int pred_kind;             /* OCT_EVAL_PRED_* */
  int has_ignore;
  int64_t ignore_index;
} OctSegEvalDesc;
int oct_seg_eval_update(const OctSegEvalDesc* d, const void* target, const void* pred, int64_t* state, void* stream);

/* Contour metrics (library 0.2.2, same OCT_VERSION): the exact integers behind Hausdorff, HD95 and ASSD of every class of a
 * (target, prediction) pair of class maps [images][h][w], uint8 (elem 0) or int64 (elem 2) each.
 * Contour points of a mask M: the midpoints of the in-image pairs of 4-adjacent pixels with exactly one pixel in M (the
 * vertices of marching squares at level 0.5); none along the image border.  M_c = {label == c}; a pixel whose TARGET equals
 * ignore_index is outside the image in both maps (a pair that touches it yields no point); labels outside [0, classes)
 * belong to no class.  In doubled coordinates (2y, 2x+1) / (2y+1, 2x) every point is integral: D2 = squared distance there
 * (true distance sqrt(D2) / 2 pixels), D2 < 2^31 because h, w <= 16384.
 *   records  int64 [images][classes][2][5], WRITTEN (not accumulated).  Direction 0: from every point of pred to the nearest
 *            point of target; direction 1 the reverse.  Per (image, class, direction):
 *            [0] n       source points
 *            [1] max_d2  largest D2
 *            [2] lo_d2   the D2 of rank lo = (19 * (n - 1)) / 20 (0-based, ascending)
 *            [3] hi_d2   the D2 of rank min(lo + 1, n - 1)
 *            [4] sum_q   sum of floor(2^16 * sqrt(D2)), every term exact
 *            n == 0 or no point on the other side: [1..4] are 0.
 *   workspace  oct_contour_workspace_bytes(d) bytes on the device, 16-byte aligned, contents irrelevant before and after:
 *            with Hd = 2h-1, Wd = 2w-1, S = Hd*Wd, G = ceil(Hd/64), each term rounded up to 256 bytes:
 *            2*images*h*w + 4*images*classes*S + 16*images*classes*G*Wd + 16*images*(S/2) + 8*images*classes
 *            + 32*images*classes + 4096*images*classes.  0 for a descriptor that oct_contour_update rejects.
 * A fixed sequence of launches on `stream`; no allocation, no host synchronisation, integer atomics only: two runs give the
 * same bits.  images * h * w < 2^31.                                                                                   */
typedef struct {
  int images, h, w, classes; /* images = product of all leading dims; 1 <= classes <= 16; h, w <= 16384 */
  int target_elem;           /* 0 uint8, 2 int64 */
  int pred_elem;             /* 0 uint8, 2 int64 */
  int has_ignore;
  int64_t ignore_index;
} OctContourDesc;
size_t oct_contour_workspace_bytes(const OctContourDesc* d);
int oct_contour_update(const OctContourDesc* d, const void* target, const void* pred, int64_t* records, void* workspace,
                       void* stream);

/* Score evaluator (library 0.2.2, same OCT_VERSION): ONE launch per batch ADDS, per channel of a binary / multi-label head,
 * the histogram of a 16-bit order-preserving key of every score, split by the element's label, to a device-resident state.
 * ROC AUC (ties counted half), average precision and the confusion counts at every threshold follow from it on the host.
 *   key16(v), v a non-NaN float32: the order-preserving code of v rounded toward -inf onto the bf16 grid.
 *           u = bits(v), h = u >> 16, low = u & 0xFFFF
 *           sign clear:  key = 0x8000 + h
 *           sign set:    m = (h & 0x7FFF) + (low != 0), capped at 0x7F80;  key = 0x8000 - m
 *           -0.0 and +0.0 share key 0x8000; keys lie in [0x0080, 0xFF80]; bin k is the half-open interval [g(k), g(k+1)) of the
 *           real line, g(k) the bf16 value of code k.  For a threshold theta on the bf16 grid v >= theta <=> key16(v) >=
 *           key16(theta) for every fp32 v, negative theta included (hence rounding toward -inf, not truncation); theta = 0 is
 *           on the grid.  bf16 and uint8 scores convert to float32 exactly: one key space for all inputs.  No fp16.
 *   target  uint8 [images][channels][h][w], values 0 / 1 (and ignore_value)
 *   scores  the same shape, planar; score_elem OCT_SCORE_F32 / _BF16 / _U8
 *   state   int64[oct_score_eval_state_elems(channels)], zeroed ONCE by the caller, C = channels:
 *           hist[C][2][65536] | nan[C] | ignored[C] | invalid[C] | updates
 *           Each element goes to exactly one place, decided in this order:
 *             has_ignore and t == ignore_value -> ignored[c];  t > 1 -> invalid[c];  the score is NaN -> nan[c];
 *             otherwise hist[c][t][key16(score)].   updates += 1 per call; images == 0 only counts the update.
 * Counts gather in LDS; one 64-bit integer atomicAdd per non-zero bin and flush, integer atomics only: two runs give the same
 * bits.  No allocation, no host synchronisation, only `stream`.  Any h, w >= 1 and any element-aligned base are accepted
 * (16-byte loads only where base and plane size allow them); images * channels * h * w < 2^31.                          */
#define OCT_SCORE_F32 0
#define OCT_SCORE_BF16 1
#define OCT_SCORE_U8 2
typedef struct {
  int images, h, w, channels; /* 1 <= channels <= OCT_MAX_CLASSES; images*channels*h*w < 2^31 */
  int score_elem;             /* OCT_SCORE_* */
  int has_ignore;
  int ignore_value;           /* in [2,255], as oct_bce_loss_* */
} OctScoreEvalDesc;
size_t oct_score_eval_state_elems(int channels); /* channels*(2*65536 + 3) + 1; 0 for channels outside 1..16 */
int oct_score_eval_update(const OctScoreEvalDesc* d, const uint8_t* target, const void* scores, int64_t* state, void* stream);

/* Paired image / label augmentation (library 0.2.2, same OCT_VERSION): ONE launch per batch warps the image, the label planes
 * and the pixel-weight map of a batch with the same per-sample geometry and runs the intensity stages on the image.  A pure
 * function of its inputs: (seed, step, sample_base + b) decide the noise, nothing else does.
 *   Geometry, fixed point.  Pixel centres at integer coordinates; output pixel (xo, yo) of the ho x wo output reads the
 *   hs x ws source at   SX = a*xo + b*yo + c + DX,   SY = d*xo + e*yo + f + DY   (Q24, evaluated in int64; sizes <= 8192).
 *   a b d e are int32 Q24 (|value| < 128, 8 is plenty); c and f are int64 Q24, |value| < 2^40 -- the offset of a flip is
 *   (ws - 1) * 2^24 and does not fit 32 bits.  Crop and resize are this map with ho x wo != hs x ws.
 *   Elastic term (OCT_AUG_ELASTIC): disp int32 Q24 [batch][2][gh][gw] (plane 0 = DX, 1 = DY), |value| <= 64 * 2^24, on a
 *   control grid of pitch P = grid_pitch = 2^k <= 1024; node (i, j) sits at output pixel (j*P, i*P), gw = ceil((wo-1)/P) + 1,
 *   gh likewise.  With j = xo >> k, rx = xo & (P-1), i = yo >> k, ry = yo & (P-1):
 *     top = n[i][j]*(P-rx) + n[i][j+1]*rx,  bot = n[i+1][j]*(P-rx) + n[i+1][j+1]*rx,  D = (top*(P-ry) + bot*ry) >> 2k
 *   (arithmetic shift, int64; a node index past the grid only occurs with weight 0 and is clamped).
 *   Sampling.  ix = SX >> 24, wx = ((SX >> 8) & 0xFFFF) * 2^-16; nearest index (SX + 2^23) >> 24; likewise for y.
 *   image   src [batch][cin][hs][ws], uint8 / bf16 / fp32 (src_elem) -> out [batch][cin][ho][wo], bf16 / fp32 (out_elem):
 *           v = (1-wy)*((1-wx)*p00 + wx*p01) + wy*((1-wx)*p10 + wx*p11), every multiply and add rounded to fp32 on its own
 *           (no fma); a tap outside the source reads `fill` (finite).  Then, with the sample's parameters:
 *             v = v*gain + bias                                   (two roundings)
 *             OCT_AUG_GAMMA:  v = exp2(gamma * log2(min(max(v, 0), 1))), 0 -> 0          (v_log_f32 / v_exp_f32)
 *             OCT_AUG_NOISE:  v = v*(1 + sigma_speckle*z1) + sigma_add*z2
 *             v = min(max(v, out_lo), out_hi), rounded to out_elem (bf16: nearest even)
 *           A stage whose flag is clear is skipped, not run with neutral values: without the two flags the path is exact.
 *           Noise: Philox4x32-10, key (seed_lo, seed_hi), counter ((yo*wo + xo) >> 1, channel, sample_base + b, step); the even
 *           pixel of a pair takes words 0,1, the odd one words 2,3:  u1 = ((w >> 9) + 0.5) * 2^-23, u2 = (w' >> 9) * 2^-23,
 *           (z1, z2) = sqrt(-2 ln u1) * (cos, sin)(2 pi u2) on v_log_f32 / v_sqrt_f32 / v_cos_f32 / v_sin_f32.
 *           cin == 0: no image (src / out may be null).
 *   weight  optional fp32 [batch][hs][ws] -> weight_out [batch][ho][wo]: the same blend, outside taps read 0, no intensity.
 *   labels  nearest, outside reads label_fill.  label_kind OCT_AUG_LABEL_CLASS_U8 / _CLASS_I64: class map [batch][hs][ws] ->
 *           labels_out int64 [batch][ho][wo];  OCT_AUG_LABEL_MASK_U8: uint8 [batch][label_planes][hs][ws] -> uint8
 *           [batch][label_planes][ho][wo], label_fill in [0, 255].
 *   params  [batch][OCT_AUG_PARAM_WORDS] 32-bit words, 8-byte aligned, per sample:
 *           [0..3] a b d e (int32)   [4,5] c, [6,7] f (int64, low word first)
 *           [8..14] gain bias gamma sigma_speckle sigma_add out_lo out_hi (fp32)   [15] unused
 * Every source index is clamped into its plane before the load.  Vector stores (8 - 16 B per thread) where wo % 4 == 0 and
 * every output base is 16-byte aligned, element-wise stores otherwise: any wo, any element-aligned base, any batch up to
 * 65535 samples.  No allocation, no synchronisation, only `stream`.  No z-score (it needs a reduction pass),
 * no 3-D volumes.                                                                                                       */
#define OCT_AUG_U8 0
#define OCT_AUG_BF16 1
#define OCT_AUG_F32 2
#define OCT_AUG_LABEL_NONE 0
#define OCT_AUG_LABEL_CLASS_U8 1
#define OCT_AUG_LABEL_CLASS_I64 2
#define OCT_AUG_LABEL_MASK_U8 3
#define OCT_AUG_GAMMA 1
#define OCT_AUG_NOISE 2
#define OCT_AUG_ELASTIC 4
#define OCT_AUG_PARAM_WORDS 16
typedef struct {
  int batch, cin;        /* cin may be 0 (labels / weight map only) */
  int hs, ws, ho, wo;    /* 1..8192 each */
  int src_elem;          /* OCT_AUG_U8 / _BF16 / _F32 */
  int out_elem;          /* OCT_AUG_BF16 / _F32 */
  int label_kind;        /* OCT_AUG_LABEL_* */
  int label_planes;      /* planes of a mask; ignored for a class map */
  int flags;             /* OCT_AUG_GAMMA | OCT_AUG_NOISE | OCT_AUG_ELASTIC */
  int grid_pitch;        /* P, a power of two in [1, 1024]; read with OCT_AUG_ELASTIC only */
  uint32_t seed_lo, seed_hi, step, sample_base;
  float fill;
  int reserved;
  int64_t label_fill;
} OctAugmentDesc;
int oct_augment_pair(const OctAugmentDesc* d, const void* src, const void* labels, const float* weight, const void* params,
                     const int32_t* disp, void* out, void* labels_out, float* weight_out, void* stream);
/* out[i][0..3] = Philox4x32-10(counter = counters[i][0..3], key = (key_lo, key_hi)): the generator of oct_augment_pair, exported
 * so that it can be pinned bit for bit.  n < 2^31.                                                                      */
int oct_augment_philox_words(const uint32_t* counters, size_t n, uint32_t key_lo, uint32_t key_hi, uint32_t* out, void* stream);

/* Connected components (library 0.2.2, same OCT_VERSION): multi-valued labelling of class maps [images][h][w], uint8 (elem 0) or
 * int64 (elem 2), a cleanup filter on the components and streaming lesion-wise detection counts.  All integer arithmetic; every
 * result is a pure function of the inputs: two runs give the same bits.
 *   outside    a pixel whose value is not in [0, classes), or (has_ignore) equals ignore_index
 *   connected  two inside pixels with the SAME value that are 4-neighbours (connectivity 4) or 8-neighbours (connectivity 8):
 *              one pass labels every class; the background's components (the "holes") come with it
 *
 * oct_cc_label(d, map, roots, info, workspace, stream)
 *   roots  int32 [images][h][w], WRITTEN: the smallest y*w + x of the pixel's component (its root); -1 for an outside pixel.
 *          Independent of scheduling; ascending root order per class is the numbering of scipy.ndimage.label.
 *   info   int32 [images][h][w], WRITTEN: at a root pixel area | (touches_border << 30), 0 everywhere else.  area < 2^29 since
 *          h*w <= 2^28; touches_border: some pixel of the component lies in row 0, row h-1, column 0 or column w-1.
 *
 * oct_cc_filter(d, rules, map, roots, info, out, workspace, stream)
 *   ONE pass over the components of the input (roots / info as oct_cc_label wrote them for `map` and `d`); no iteration to a
 *   fixed point.  A component of class c is REPLACED when
 *     area < min_area[c]  (0 = off; area == min_area is kept), or
 *     keep_largest[c] and it is not the image's component of class c with the greatest area, ties to the smallest root (one
 *       64-bit atomicMax per component on the key area << 32 | (0xFFFFFFFF - root): in LDS per workgroup, the workgroup's
 *       maximum then into a per-(image, class) workspace slot), or
 *     drop_enclosed[c] and it does not touch the border.
 *   Replaced pixels get replace[c]; all other pixels, outside ones included, are copied.  `out` has the element type of `map` and
 *   may be `map` itself.  Filling the holes of a binary mask: drop_enclosed[0] = 1, replace[0] = 1.  `rules` is host memory.
 *
 * oct_lesion_eval_update(d, target, pred, state, workspace, stream)        (streaming, like oct_seg_eval_update)
 *   A pixel whose TARGET equals ignore_index is outside in BOTH maps (the rule of oct_contour_update): such a pixel splits a
 *   predicted component that runs through it.  Both maps are labelled.  For a target component G of class c
 *     inter(G) = #{pixels of G with pred == c};   G is DETECTED when inter(G) >= 1 and inter(G) * den >= num * area(G)
 *   (num / den = overlap_num / overlap_den, the minimum overlap fraction, 0 <= num <= den, den >= 1; products in 64 bits).  A
 *   predicted component is CONFIRMED by the same rule with the roles swapped.
 *   state  int64 [classes][4] + 4, zeroed ONCE by the caller and ADDED to:
 *          [c*4 + 0..3]   target components, predicted components, detected, confirmed of class c
 *          [classes*4 +]  images, ignored pixels, invalid pixels (not ignored, t or p outside [0, classes)), updates
 *
 * workspace  oct_cc_workspace_bytes(d) bytes on the device for d->op, 16-byte aligned, contents irrelevant before and after.
 *            With N = images*h*w and A(x) = x rounded up to 256:
 *              OCT_CC_OP_LABEL   A(N)                               the classes as bytes
 *              OCT_CC_OP_FILTER  A(N) + A(8*images*classes)         enough for a label and the filter behind it
 *              OCT_CC_OP_LESION  2*A(N) + 6*A(4*N)                  bytes, roots, info and inter of both maps
 *            0 for a descriptor that the entry points reject.  Each entry point uses the layout of its own op whatever d->op.
 * oct_cc_tile  the tile (rows, columns) of the local pass: shapes that straddle tile borders follow from it.
 * Launches: one workgroup per tile runs union-find in LDS (row runs by wave ballot) and writes every pixel's parent and each
 * tile-local component's area; a border pass unites across the tile edges (and the diagonals, connectivity 8) with agent-scope
 * atomicMin whose return value decides; a flatten pass writes the roots and adds the tile-local areas at the root.  No
 * workgroup waits on another; parents only decrease, so every walk ends.  No allocation, no host synchronisation,
 * integer atomics only, only `stream`.  Any h, w in 1..16384, any element-aligned base (read element-wise); images*h*w < 2^31. */
#define OCT_CC_OP_LABEL 0
#define OCT_CC_OP_FILTER 1
#define OCT_CC_OP_LESION 2
#define OCT_CC_BORDER_BIT 30 /* info: area | touches_border << 30 */
typedef struct {
  int images, h, w, classes; /* images = product of all leading dims; 1 <= classes <= 16; h, w <= 16384 */
  int map_elem;              /* 0 uint8, 2 int64: the map (label, filter) or the target (lesion) */
  int pred_elem;             /* 0 uint8, 2 int64: the prediction (lesion); 0 otherwise */
  int connectivity;          /* 4 or 8 */
  int op;                    /* OCT_CC_OP_*: which workspace oct_cc_workspace_bytes sizes */
  int has_ignore;
  int overlap_num, overlap_den; /* lesion: minimum overlap fraction, 0 <= num <= den, den >= 1 (0 / 1: any overlap) */
  int reserved;
  int64_t ignore_index;
} OctCcDesc;
typedef struct {
  int min_area[OCT_MAX_CLASSES];      /* 0 = off */
  int keep_largest[OCT_MAX_CLASSES];  /* 0 / 1 */
  int drop_enclosed[OCT_MAX_CLASSES]; /* 0 / 1 */
  int64_t replace[OCT_MAX_CLASSES];   /* uint8 maps: 0..255 */
} OctCcRules;
size_t oct_cc_workspace_bytes(const OctCcDesc* d);
int oct_cc_tile(int* th, int* tw);
int oct_cc_label(const OctCcDesc* d, const void* map, int32_t* roots, int32_t* info, void* workspace, void* stream);
int oct_cc_filter(const OctCcDesc* d, const OctCcRules* rules, const void* map, const int32_t* roots, const int32_t* info, void* out,
                  void* workspace, void* stream);
int oct_lesion_eval_update(const OctCcDesc* d, const void* target, const void* pred, int64_t* state, void* workspace, void* stream);

/* Distance maps (library 0.2.2, same OCT_VERSION): the exact squared Euclidean distance, in pixels, from every pixel of a class
 * map [images][h][w], uint8 (elem 0) or int64 (elem 2), to the nearest site of each of a list of planes, and the two maps a
 * training step makes of it.  All integer arithmetic up to the epilogue; every result is a pure function of the inputs: two runs
 * give the same bits.
 *   valid      a pixel whose value is in [0, classes) and (has_ignore) is not ignore_index.  An invalid pixel is a site of no
 *              plane; it still receives a distance
 *   sites      OCT_DT_BOUNDARY  valid pixels with a 4-neighbour INSIDE THE IMAGE that is valid and has another value (the image
 *                               edge is no boundary, an invalid neighbour makes none)
 *              OCT_DT_CLASS c   valid pixels equal to c            OCT_DT_OTHER c   valid pixels not equal to c
 *   D2         int32: min over the sites (ys, xs) of the image of (y - ys)^2 + (x - xs)^2; 0 on a site; OCT_DT_FAR everywhere in
 *              an image whose plane has no site.  h, w <= 16384 keeps every real value below OCT_DT_FAR
 *
 * oct_dt_squared(d, planes, map, out, workspace, stream)
 *   planes  HOST memory, int32 [d->planes][2] = (OCT_DT_BOUNDARY / _CLASS / _OTHER, class); class in [0, classes), 0 for a
 *           boundary plane.  1 <= d->planes <= OCT_DT_MAX_PLANES
 *   out     int32 [images][planes][h][w], WRITTEN: D2
 * oct_dt_weight_map(d, planes, map, table, table_len, out, workspace, stream)
 *   table   fp32 [table_len] on the device, table_len >= 1, indexed by the SQUARED distance
 *   out     fp32 [images][planes][h][w], WRITTEN: table[min(D2, table_len - 1)] -- a copy of the entry, so any profile of the
 *           distance tabulated on the host is reproduced bit for bit; no int32 plane is written
 * oct_dt_signed(d, class_ids, map, out, workspace, stream)
 *   class_ids  HOST memory, int32 [d->planes], each in [0, classes); d->planes <= OCT_DT_MAX_PLANES / 2
 *   out     fp32 [images][planes][h][w], WRITTEN: on a pixel of class c  -sqrtf(D2 to OCT_DT_OTHER c), on every other pixel
 *           (invalid ones included)  +sqrtf(D2 to OCT_DT_CLASS c); the whole plane of an image is 0 where the class is absent
 *           or nothing valid lies outside it.  D2 is converted to fp32 (exact below 2^24) and sqrtf is IEEE: one rounding
 *
 * workspace  oct_dt_workspace_bytes(d) bytes on the device for d->op, 16-byte aligned, contents irrelevant before and after.
 *            With N = images*h*w, G = planes (signed: 2*planes), S = ceil(h/64) and A(x) = x rounded up to 256:
 *              [A(N) for an int64 map] + A(2*G*N) + A(8*G*images*S*w) + A(4*G*images)
 *            the map as bytes, the column distances, the column masks, the has-a-site flags.  0 for a descriptor the entry
 *            points reject.  Each entry point uses the layout of its own op whatever d->op.
 * oct_dt_block  rows: the rows one column-pass thread covers (one 64-bit site mask); cols: the pixels one row-pass workgroup
 *            covers (whole rows where rows are shorter than that, a stretch of one row otherwise).  Shapes that straddle either
 *            follow from it.
 * Launches: [labels, int64 only] -> column masks -> column distances g (uint16) -> rows: the g rows of a workgroup in LDS in
 * blocks of 16 columns with each block's smallest g; D2(x) = min over x' of (x - x')^2 + g[x']^2, taken over the columns next to
 * x, then block by block outward while a block's nearest column is closer than sqrt(best), reading a block only where that
 * distance squared plus its smallest g squared is below best: every column that could lower the minimum is read.
 * A value is range-checked before it indexes anything.  The one atomic is the flag's atomicOr.  No allocation, no host
 * synchronisation, only `stream`.  Any h, w in 1..16384, any element-aligned base; images*h*w < 2^31; images == 0 is a no-op. */
#define OCT_DT_FAR (1 << 30)
#define OCT_DT_MAX_PLANES 64
#define OCT_DT_BOUNDARY 0
#define OCT_DT_CLASS 1
#define OCT_DT_OTHER 2
#define OCT_DT_OP_SQUARED 0
#define OCT_DT_OP_WEIGHT 1
#define OCT_DT_OP_SIGNED 2
typedef struct {
  int images, h, w, classes; /* images = product of all leading dims; 1 <= classes <= 16; h, w <= 16384 */
  int map_elem;              /* 0 uint8, 2 int64 */
  int has_ignore;
  int planes;                /* planes of the output: the plane list, or the class list of oct_dt_signed */
  int op;                    /* OCT_DT_OP_*: which workspace oct_dt_workspace_bytes sizes */
  int64_t ignore_index;
} OctDtDesc;
size_t oct_dt_workspace_bytes(const OctDtDesc* d);
int oct_dt_block(int* rows, int* cols);
int oct_dt_squared(const OctDtDesc* d, const int32_t* planes, const void* map, int32_t* out, void* workspace, void* stream);
int oct_dt_weight_map(const OctDtDesc* d, const int32_t* planes, const void* map, const float* table, int table_len, float* out,
                      void* workspace, void* stream);
int oct_dt_signed(const OctDtDesc* d, const int32_t* class_ids, const void* map, float* out, void* workspace, void* stream);

/* Layer surfaces (library 0.2.2, same OCT_VERSION): the K - 1 ordered boundary rows per A-scan between K classes listed top to
 * bottom, from a class map [images][h][w] (uint8: elem 0, int64: elem 2) or from scores [images][classes][h][w] (NCHW; fp32:
 * elem 3, bf16: elem 4, widened to fp32 first).  Exact integers: every result is a pure function of the inputs.
 *   order     K distinct classes, 2 <= K <= OCT_SURF_MAX_K, top to bottom
 *   free      map: a value not in order, equal to ignore_index (has_ignore) or outside [0, classes);  scores: any channel NaN.
 *             A free pixel costs nothing wherever a surface passes
 *   u_j(y,x)  j = 0..K-1.  map: 0 on a free pixel or where the class is order[j], else 1.  scores: with m the maximum over ALL
 *             channels, v = (m - z[order[j]]) * scale + 0.5 in fp32, every operation rounded on its own (no FMA), the
 *             difference taken as 0 where z == m;  u_j = floor(v) if v < qmax + 1, else qmax;  0 on a free pixel
 *   surface k k = 1..K-1 splits order[:k] | order[k:]:  d_k(y,x) = min_{j<k} u_j - min_{j>=k} u_j,
 *             N_k(x,s) = sum_{y<s} d_k(y,x) for s = 0..h (the rows y < s lie above the surface)
 *   path      s_k(0..w-1) with |s_k(x+1) - s_k(x)| <= max_step minimising sum_x N_k(x, s_k(x)), chosen by exactly
 *               A(0,s) = N(0,s);  A(x,s) = N(x,s) + min A(x-1,t) over |t-s| <= max_step, 0 <= t <= h;  P(x,s) = the SMALLEST
 *               such t;  s(w-1) = the smallest argmin of A(w-1,.);  s(x-1) = P(x, s(x))
 *             max_step = -1 (none): s(x) = the smallest argmin of N(x,.)
 *   ordering  afterwards s_k <- max(s_k, s_{k-1}) down the surfaces (a tie-breaker: DESIGN.md)
 *   painted   out(y,x) = order[#{k : s_k(x) <= y}]; where the input class (scores: the arg-max, first maximum, the first NaN
 *             beats everything) is listed in `keep` (disjoint from order) the pixel keeps it
 *
 * oct_surf_extract(d, order, in, surfaces, workspace, stream)
 *   order     HOST memory, int32 [d->k]
 *   surfaces  int32 [images][k-1][w], WRITTEN, values in [0, h]
 *   workspace oct_surf_workspace_bytes(d) bytes on the device, 16-byte aligned, contents irrelevant before and after: with
 *             cells = images*(k-1)*w*(h+1) and A(x) = x rounded up to 256, A(4*cells) + A(cells): N as int32 [image][k][x][s]
 *             and P as int8 offsets t - s.  0 (and no workspace is read) with max_step = -1; 0 too for a descriptor the entry
 *             points reject
 * oct_surf_paint(d, order, keep, in, surfaces, out, stream)
 *   keep      HOST memory, int32 [d->nkeep], null with nkeep = 0
 *   in        read only where nkeep > 0 (scores) / always validated (maps: it fixes the output's element)
 *   out       [images][h][w], the map's element, int64 for scores, WRITTEN; may be `in` itself for a map (one read, one write per
 *             pixel by the same thread)
 * oct_surf_error_update(d, target_surf, pred_surf, valid, state, stream)
 *   uses d->images, d->w, d->k only.  valid: uint8 [images][w] or null (every column).  state: int64 [k-1][5], ADDED TO:
 *   count, sum |e|, sum e, sum e^2 and (atomicMax) max |e| with e = pred - target over the valid columns.  The rows are
 *   expected in [0, OCT_SURF_MAX_H], as oct_surf_extract writes them: the sums are then exact; they are not range-checked
 *
 * Refused: h > OCT_SURF_MAX_H; qmax * h * w >= 2^31 (a map counts as qmax = 1): every path cost fits int32; max_step outside
 * -1..OCT_SURF_MAX_STEP; scale not finite and positive; qmax outside 1..255; order / keep entries outside [0, classes), repeated
 * in order, or shared between the two.  Launches: cost (unary bytes through LDS, a wave scan per column and surface; with
 * max_step = -1 it keeps each column's arg-min, writes `surfaces` and nothing else runs) -> search (one workgroup per (image,
 * surface), A in two LDS rows, one barrier per column, then the walk back) -> ordering.  No allocation, no host
 * synchronisation, no floating-point atomics, only `stream`; images == 0 is a no-op. */
#define OCT_SURF_MAX_K 16
#define OCT_SURF_MAX_H 4095
#define OCT_SURF_MAX_STEP 32
typedef struct {
  int images, h, w, classes; /* images = product of all leading dims; classes = channels of scores; 1 <= classes <= 16 */
  int elem;                  /* 0 uint8 map, 2 int64 map, 3 fp32 scores, 4 bf16 scores */
  int k;                     /* entries of order */
  int max_step;              /* -1: none */
  int has_ignore;            /* maps */
  int nkeep;                 /* entries of keep (oct_surf_paint) */
  int qmax;                  /* scores: 1..255 */
  float scale;               /* scores: finite, > 0 */
  int reserved;
  int64_t ignore_index;
} OctSurfDesc;
size_t oct_surf_workspace_bytes(const OctSurfDesc* d);
int oct_surf_extract(const OctSurfDesc* d, const int32_t* order, const void* in, int32_t* surfaces, void* workspace, void* stream);
int oct_surf_paint(const OctSurfDesc* d, const int32_t* order, const int32_t* keep, const void* in, const int32_t* surfaces, void* out,
                   void* stream);
int oct_surf_error_update(const OctSurfDesc* d, const int32_t* target_surf, const int32_t* pred_surf, const uint8_t* valid,
                          int64_t* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OCT_HIP_H */
