// Cross-entropy + soft-Dice loss on logits that a network has already produced (U_Net, AttU_Net, MGU-Net, ReLayNet: every
// network whose class head is not the fused UNet head of head.hip).  Two layouts, one per-pixel code path:
//   NHWC in the compute dtype (what the networks write) -- a block's 256 pixels are one contiguous span of 256 * classes
//     elements: it is staged through LDS with 16-B loads (and d(loss)/d(logits) leaves the same way), so a 3-class bf16 row of
//     6 B never turns into 2-B scalar accesses;
//   NCHW fp32 (what every network's forward returns) -- per class, consecutive lanes read consecutive addresses.
// The forward writes per-workgroup fp64 rows in head_fwd_kernel's layout [OCT_HEAD_LOSS_SLOTS], so oct_head_loss_finalize
// turns them into [loss, ce, dice] and the Dice backward coefficients unchanged.  The reduction order is fixed: per-lane sums,
// wave sums, workgroup sums, one row per workgroup -- no atomics.
// The weighted forms (WEIGHTED = true; oct_seg_loss_*_weighted) scale each pixel's cross-entropy by
//   omega = [t != ignore_index] * class_weight[t] * pixel_weight[pixel]
// and divide by sum(omega) instead of N; the Dice sums and gradients run over the pixels that are not ignored.  sum(omega)
// needs the labels and the map only, so it is reduced first (seg_wsum_kernel) or carried in slot 1 of the forward rows, stays
// on the device, and the backward kernel reads it there the way it reads *dloss: no host synchronisation, fixed order.
// The unweighted instantiations are the code they were: every weighted statement sits behind `if constexpr (WEIGHTED)`.
#include "common.h"

#define SEG_THREADS 256
#define SEG_MAX_GRID 1024

struct SegParams {
  const void* logits; const int64_t* target; int64_t* argmax; double* loss_partials;
  const float* dice_coef; const float* dloss; void* dlogits; float w_ce;
  size_t npix, hw; int classes; int vec_in, vec_out;
  // weighted forms only (each may be null / off)
  const float* class_weight; const float* pixel_weight; const double* wsum; double* wsum_partials;
  long long ignore_index; int has_ignore;
};

// one tile = SEG_THREADS consecutive pixels, one per lane.  NHWC: the tile's span of the tensor goes through `stage` with
// 16-B accesses (the span starts 16-B aligned: 256 * classes * sizeof(T) is a multiple of 16; vec = base pointer aligned too)
template <typename T>
__device__ __forceinline__ void stage_copy(T* __restrict__ dst, const T* __restrict__ src, int ne, bool vec) {
  int done = 0;
  if (vec) {
    const int nq = (int)((ne * sizeof(T)) >> 4);
    for (int i = threadIdx.x; i < nq; i += SEG_THREADS)
      reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    done = (int)((nq * 16) / sizeof(T));
  }
  for (int i = done + threadIdx.x; i < ne; i += SEG_THREADS) dst[i] = src[i];
}

template <bool NCHW, typename T, int CMAX>
__device__ __forceinline__ void seg_load(const SegParams& p, size_t p0, int np, T* stage, float (&l)[CMAX]) {
  const int C = p.classes;
  const size_t pix = p0 + threadIdx.x;
  const bool live = threadIdx.x < np;
  if (NCHW) {
    const float* x = reinterpret_cast<const float*>(p.logits);
    const size_t img = live ? pix / p.hw : 0, off = live ? pix - img * p.hw : 0;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) l[c] = (live && c < C) ? x[(img * C + c) * p.hw + off] : 0.f;
  } else {
    stage_copy<T>(stage, reinterpret_cast<const T*>(p.logits) + p0 * C, np * C, p.vec_in);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CMAX; ++c) l[c] = (live && c < C) ? to_f32(stage[threadIdx.x * C + c]) : 0.f;
  }
}

template <int CMAX>
__device__ __forceinline__ void seg_softmax(int classes, const float (&l)[CMAX], float (&pr)[CMAX], float& m, float& lse) {
  m = l[0];
#pragma unroll
  for (int c = 1; c < CMAX; ++c)
    if (c < classes) m = fmaxf(m, l[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    pr[c] = (c < classes) ? expf(l[c] - m) : 0.f;
    s += pr[c];
  }
  const float inv = 1.f / s;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) pr[c] *= inv;
  lse = logf(s);
}

// -log softmax[t] of one pixel; NaN for a label outside [0, classes) (torch's nll_loss raises there; no synchronisation here)
template <int CMAX>
__device__ __forceinline__ float seg_ce(int classes, int t, const float (&l)[CMAX], float m, float lse) {
  float lt = 0.f;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) lt = (c == t) ? l[c] : lt;
  return (unsigned)t < (unsigned)classes ? -(lt - m - lse) : __builtin_nanf("");
}

// wave -> workgroup -> one fp64 row per workgroup (head_fwd_kernel's layout: [ce, 0, I_c..., P_c..., Y_c...])
// WEIGHTED: slot 1 carries the workgroup's sum of omega (ws)
template <int CMAX, bool WEIGHTED = false>
__device__ __forceinline__ void seg_write_row(double* __restrict__ row, float ce, const float (&si)[CMAX], const float (&sp)[CMAX],
                                              const float (&sy)[CMAX], bool dice, double (&red)[SEG_THREADS / 64][OCT_HEAD_LOSS_SLOTS],
                                              double ws = 0.0) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double v = wave_sum((double)ce);
  double v1 = 0.0;
  if constexpr (WEIGHTED) v1 = wave_sum(ws);
  if (lane == 0) { red[wave][0] = v; red[wave][1] = v1; }
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    const double a = dice ? wave_sum((double)si[c]) : 0.0, b = dice ? wave_sum((double)sp[c]) : 0.0,
                 d = dice ? wave_sum((double)sy[c]) : 0.0;
    if (lane == 0) {
      red[wave][2 + c] = a; red[wave][2 + OCT_MAX_CLASSES + c] = b; red[wave][2 + 2 * OCT_MAX_CLASSES + c] = d;
    }
  }
  if (lane == 0)
    for (int c = CMAX; c < OCT_MAX_CLASSES; ++c) {
      red[wave][2 + c] = 0.0; red[wave][2 + OCT_MAX_CLASSES + c] = 0.0; red[wave][2 + 2 * OCT_MAX_CLASSES + c] = 0.0;
    }
  __syncthreads();
  for (int i = threadIdx.x; i < OCT_HEAD_LOSS_SLOTS; i += SEG_THREADS) {
    double s = 0.0;
    for (int wv = 0; wv < SEG_THREADS / 64; ++wv) s += red[wv][i];
    row[i] = s;
  }
}

template <typename T, int CMAX>
struct SegStage { T v[SEG_THREADS * CMAX]; };

// class weights: <= 16 floats, once per workgroup into LDS (1 everywhere without them)
__device__ __forceinline__ void seg_load_class_weights(const SegParams& p, float* scw) {
  if (threadIdx.x < OCT_MAX_CLASSES)
    scw[threadIdx.x] = (p.class_weight && (int)threadIdx.x < p.classes) ? p.class_weight[threadIdx.x] : 1.f;
  __syncthreads();
}

// omega of one live pixel and whether it counts at all; the map is read one float per lane next to the label.  A label outside
// [0, classes) that is not the ignored one keeps weight 1: its cross-entropy is NaN whatever the weight.
__device__ __forceinline__ float seg_omega(const SegParams& p, const float* scw, size_t pix, long long t64, bool& valid) {
  valid = !(p.has_ignore && t64 == p.ignore_index);
  const float pw = p.pixel_weight ? p.pixel_weight[pix] : 1.f;
  const float cw = (unsigned long long)t64 < (unsigned long long)p.classes ? scw[(int)t64] : 1.f;
  return valid ? cw * pw : 0.f;
}

template <bool NCHW, typename T, int CMAX, bool WEIGHTED = false>
__global__ void __launch_bounds__(SEG_THREADS) seg_fwd_kernel(const SegParams p) {
  __shared__ __attribute__((aligned(16))) SegStage<T, NCHW ? 1 : CMAX> stage;
  __shared__ double red[SEG_THREADS / 64][OCT_HEAD_LOSS_SLOTS];
  __shared__ float scw[WEIGHTED ? OCT_MAX_CLASSES : 1];
  if constexpr (WEIGHTED) seg_load_class_weights(p, scw);
  double ws = 0.0;
  const int C = p.classes;
  float ce = 0.f, si[CMAX], sp[CMAX], sy[CMAX];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) { si[c] = 0.f; sp[c] = 0.f; sy[c] = 0.f; }
  const size_t ntiles = (p.npix + SEG_THREADS - 1) / SEG_THREADS;
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t p0 = tile * SEG_THREADS, pix = p0 + threadIdx.x;
    const int np = (int)(p.npix - p0 < SEG_THREADS ? p.npix - p0 : SEG_THREADS);
    float l[CMAX];
    seg_load<NCHW, T, CMAX>(p, p0, np, stage.v, l);
    if (threadIdx.x < np) {
      if (p.argmax) {   // on the logits, first maximum wins and NaN beats everything (torch.argmax)
        int best = 0; float bv = l[0];
#pragma unroll
        for (int c = 1; c < CMAX; ++c)
          if (c < C && (l[c] > bv || (l[c] != l[c] && bv == bv))) { bv = l[c]; best = c; }
        p.argmax[pix] = best;
      }
      if (p.loss_partials) {
        float pr[CMAX], m, lse;
        seg_softmax<CMAX>(C, l, pr, m, lse);
        if constexpr (WEIGHTED) {
          const long long t64 = p.target[pix];
          const int t = (int)t64;
          bool valid;
          const float om = seg_omega(p, scw, pix, t64, valid);
          if (valid) {   // an ignored pixel adds exactly nothing, whatever its logits and label are
            ce += om * seg_ce<CMAX>(C, t, l, m, lse);
            ws += (double)om;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
              const bool hit = (c == t);
              si[c] += hit ? pr[c] : 0.f;
              sp[c] += pr[c];
              sy[c] += hit ? 1.f : 0.f;
            }
          }
        } else {
          const int t = (int)p.target[pix];
          ce += seg_ce<CMAX>(C, t, l, m, lse);
#pragma unroll
          for (int c = 0; c < CMAX; ++c) {
            const bool hit = (c == t);
            si[c] += hit ? pr[c] : 0.f;
            sp[c] += pr[c];
            sy[c] += hit ? 1.f : 0.f;
          }
        }
      }
    }
    if (!NCHW) __syncthreads();   // the next tile overwrites the stage
  }
  if (p.loss_partials)
    seg_write_row<CMAX, WEIGHTED>(p.loss_partials + (size_t)blockIdx.x * OCT_HEAD_LOSS_SLOTS, ce, si, sp, sy, true, red, ws);
}

// d(loss)/d(logits) = g * [w_ce (p - onehot) / N + p (dp - <p, dp>)], dp_c = A_c [c == t] + B_c from the finalize kernel's
// dice_coef (no Dice term without it) -- oct_head_dlogits's formula; g = *dloss (1 without it), read here so that an autograd
// backward never synchronises.  loss_partials (only without a Dice term): the CE rows as well, so the CE-only step reads the
// logits once.
// WEIGHTED: w_ce (p - onehot) omega / sum(omega) with sum(omega) = *wsum read from the device, the Dice term on the pixels that
// are not ignored, exactly 0 in every class of an ignored pixel; the CE rows then carry sum(omega * ce) and sum(omega).
template <bool NCHW, typename T, int CMAX, bool WEIGHTED = false>
__global__ void __launch_bounds__(SEG_THREADS) seg_bwd_kernel(const SegParams p) {
  __shared__ __attribute__((aligned(16))) SegStage<T, NCHW ? 1 : CMAX> stage;
  __shared__ double red[SEG_THREADS / 64][OCT_HEAD_LOSS_SLOTS];
  __shared__ float scw[WEIGHTED ? OCT_MAX_CLASSES : 1];
  if constexpr (WEIGHTED) seg_load_class_weights(p, scw);
  double ws = 0.0;
  const int C = p.classes;
  float dcA[CMAX], dcB[CMAX];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    dcA[c] = (p.dice_coef && c < C) ? p.dice_coef[c] : 0.f;
    dcB[c] = (p.dice_coef && c < C) ? p.dice_coef[OCT_MAX_CLASSES + c] : 0.f;
  }
  const float g = p.dloss ? *p.dloss : 1.f;
  const float inv_n = WEIGHTED ? (float)(1.0 / *p.wsum) : 1.f / (float)p.npix;
  float ce = 0.f;
  T* out = reinterpret_cast<T*>(p.dlogits);
  const size_t ntiles = (p.npix + SEG_THREADS - 1) / SEG_THREADS;
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t p0 = tile * SEG_THREADS, pix = p0 + threadIdx.x;
    const int np = (int)(p.npix - p0 < SEG_THREADS ? p.npix - p0 : SEG_THREADS);
    float l[CMAX], pr[CMAX], dl[CMAX], m, lse;
    seg_load<NCHW, T, CMAX>(p, p0, np, stage.v, l);
    const bool live = threadIdx.x < np;
    const long long t64 = live ? p.target[pix] : 0;
    const int t = (int)t64;
    seg_softmax<CMAX>(C, l, pr, m, lse);
    if constexpr (WEIGHTED) {
      bool valid = false;
      const float om = live ? seg_omega(p, scw, pix, t64, valid) : 0.f;
      const float k = om * inv_n;   // omega / sum(omega) in the place of 1 / N, in the unweighted kernel's own expression
      float dp[CMAX], dot = 0.f;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        dp[c] = (c == t ? dcA[c] : 0.f) + dcB[c];
        dot = fmaf(pr[c], dp[c], dot);
      }
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        dl[c] = valid ? (p.w_ce * (pr[c] - (c == t ? 1.f : 0.f)) * k + pr[c] * (dp[c] - dot)) * g : 0.f;
      if (p.loss_partials && valid) {
        ce += om * seg_ce<CMAX>(C, t, l, m, lse);
        ws += (double)om;
      }
    } else {
      float dp[CMAX], dot = 0.f;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        dp[c] = (c == t ? dcA[c] : 0.f) + dcB[c];
        dot = fmaf(pr[c], dp[c], dot);
      }
#pragma unroll
      for (int c = 0; c < CMAX; ++c) dl[c] = (p.w_ce * (pr[c] - (c == t ? 1.f : 0.f)) * inv_n + pr[c] * (dp[c] - dot)) * g;
    }
    if constexpr (!WEIGHTED)
      if (p.loss_partials && live) ce += seg_ce<CMAX>(C, t, l, m, lse);
    if (NCHW) {
      if (live) {
        float* o = reinterpret_cast<float*>(p.dlogits);
        const size_t img = pix / p.hw, off = pix - img * p.hw;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
          if (c < C) o[(img * C + c) * p.hw + off] = dl[c];
      }
    } else {
      __syncthreads();   // every lane has read its logits from the stage
      if (live) {
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
          if (c < C) stage.v[threadIdx.x * C + c] = from_f32<T>(dl[c]);
      }
      __syncthreads();
      stage_copy<T>(out + p0 * C, stage.v, np * C, p.vec_out);
      __syncthreads();   // the next tile overwrites the stage
    }
  }
  if (p.loss_partials) {
    float z[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) z[c] = 0.f;
    seg_write_row<CMAX, WEIGHTED>(p.loss_partials + (size_t)blockIdx.x * OCT_HEAD_LOSS_SLOTS, ce, z, z, z, false, red, ws);
  }
}

// sum(omega) from the labels and the map alone (12 B per pixel): per-lane fp64 sums, wave, workgroup, one partial per workgroup
__global__ void __launch_bounds__(SEG_THREADS) seg_wsum_kernel(const SegParams p) {
  __shared__ float scw[OCT_MAX_CLASSES];
  __shared__ double red[SEG_THREADS / 64];
  seg_load_class_weights(p, scw);
  double ws = 0.0;
  const size_t ntiles = (p.npix + SEG_THREADS - 1) / SEG_THREADS;
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t pix = tile * SEG_THREADS + threadIdx.x;
    if (pix < p.npix) {
      bool valid;
      ws += (double)seg_omega(p, scw, pix, p.target[pix], valid);
    }
  }
  ws = wave_sum(ws);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ws;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int wv = 0; wv < SEG_THREADS / 64; ++wv) s += red[wv];
    p.wsum_partials[blockIdx.x] = s;
  }
}

// Sum of v[seg], v[seg + 16], ... (n values `stride` doubles apart) in head_loss_finalize_kernel's order: eight independent
// partial sums keep eight loads in flight instead of one dependent load per round trip, then a fixed tree.  Both reductions
// below go through it, so sum(omega) has the same bits whether it comes from seg_wsum_kernel's partials or from slot 1 of the rows.
__device__ __forceinline__ double seg_strided_sum(const double* __restrict__ v, size_t stride, int seg, int n) {
  double sv[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int b = seg;
  for (; b + 7 * 16 < n; b += 8 * 16) {
#pragma unroll
    for (int u = 0; u < 8; ++u) sv[u] += v[(size_t)(b + 16 * u) * stride];
  }
  for (; b < n; b += 16) sv[0] += v[(size_t)b * stride];
  return ((sv[0] + sv[1]) + (sv[2] + sv[3])) + ((sv[4] + sv[5]) + (sv[6] + sv[7]));
}

// the workgroup partials (<= SEG_MAX_GRID) -> one double on the device
__global__ void __launch_bounds__(64) seg_wsum_reduce_kernel(const double* __restrict__ partials, int nblocks,
                                                             double* __restrict__ wsum) {
  __shared__ double part[16];
  if (threadIdx.x < 16) part[threadIdx.x] = seg_strided_sum(partials, 1, threadIdx.x, nblocks);
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    for (int k = 0; k < 16; ++k) a += part[k];
    *wsum = a;
  }
}

// head_loss_finalize_kernel's result with CE = sum(omega * ce) / sum(omega): slot 0 over slot 1 of the rows instead of slot 0
// over N.  Same reduction order, Dice arithmetic and dice_coef; wsum_out (may be null) receives sum(omega) for the backward kernel.
__global__ void __launch_bounds__(1024) seg_finalize_weighted_kernel(const double* __restrict__ partials, int nblocks, int classes,
                                                                     float w_ce, float w_dice, float eps, float* loss_out,
                                                                     float* dice_coef, double* wsum_out) {
  __shared__ double tot[OCT_HEAD_LOSS_SLOTS];
  __shared__ double part[16][64];
  const int slot = threadIdx.x & 63, seg = threadIdx.x >> 6;
  part[seg][slot] = slot < OCT_HEAD_LOSS_SLOTS ? seg_strided_sum(partials + slot, OCT_HEAD_LOSS_SLOTS, seg, nblocks) : 0.0;
  __syncthreads();
  if (threadIdx.x < OCT_HEAD_LOSS_SLOTS) {
    double a = 0.0;
    for (int k = 0; k < 16; ++k) a += part[k][slot];
    tot[threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double ce = tot[0] / tot[1];   // everything ignored: 0 / 0 = NaN, as torch
    double dsum = 0.0;
    for (int c = 0; c < classes; ++c) {
      const double I = tot[2 + c], P = tot[2 + OCT_MAX_CLASSES + c], Y = tot[2 + 2 * OCT_MAX_CLASSES + c];
      const double den = P + Y + (double)eps, num = 2.0 * I + (double)eps;
      dsum += num / den;
      dice_coef[c] = (float)(-(double)w_dice / classes * 2.0 / den);
      dice_coef[OCT_MAX_CLASSES + c] = (float)((double)w_dice / classes * num / (den * den));
    }
    const double dice = 1.0 - dsum / classes;
    loss_out[0] = (float)((double)w_ce * ce + (double)w_dice * dice);
    loss_out[1] = (float)ce;
    loss_out[2] = (float)dice;
    if (wsum_out) *wsum_out = tot[1];
  }
}

extern "C" int oct_seg_loss_blocks(size_t npix, int classes) {
  if (npix == 0 || classes < 1 || classes > OCT_MAX_CLASSES) return 0;
  const size_t tiles = (npix + SEG_THREADS - 1) / SEG_THREADS;
  return (int)(tiles < SEG_MAX_GRID ? tiles : SEG_MAX_GRID);
}

static int seg_check(const OctHeadDesc* d, int layout, const char* who) {
  OCT_CHECK(d, "%s: null descriptor", who);
  OCT_CHECK(layout == OCT_SEG_NHWC || layout == OCT_SEG_NCHW, "%s: bad layout %d (OCT_SEG_NHWC or OCT_SEG_NCHW)", who, layout);
  OCT_CHECK(d->dtype == OCT_DT_BF16 || d->dtype == OCT_DT_F32, "%s: bad dtype %d", who, d->dtype);
  OCT_CHECK(layout == OCT_SEG_NHWC || d->dtype == OCT_DT_F32, "%s: NCHW logits are fp32 only", who);
  OCT_CHECK(d->n > 0 && d->h > 0 && d->w > 0, "%s: bad shape", who);
  OCT_CHECK(d->classes > 0 && d->classes <= OCT_MAX_CLASSES, "%s: classes %d not in [1,%d]", who, d->classes, OCT_MAX_CLASSES);
  return OCT_OK;
}

static SegParams seg_params(const OctHeadDesc* d, const void* logits) {
  SegParams p = {};
  p.logits = logits;
  p.hw = (size_t)d->h * d->w;
  p.npix = (size_t)d->n * p.hw;
  p.classes = d->classes;
  p.vec_in = ((uintptr_t)logits & 15) == 0;
  return p;
}

#define SEG_DISPATCH(KERNEL, W, d, layout, grid, s, p)                                                           \
  do {                                                                                                           \
    const int cm = (d)->classes <= 2 ? 2 : (d)->classes <= 4 ? 4 : (d)->classes <= 8 ? 8 : 16;                   \
    const dim3 gd(grid), bd(SEG_THREADS);                                                                        \
    if ((layout) == OCT_SEG_NCHW) {                                                                              \
      if (cm == 2) hipLaunchKernelGGL((KERNEL<true, float, 2, W>), gd, bd, 0, s, p);                             \
      else if (cm == 4) hipLaunchKernelGGL((KERNEL<true, float, 4, W>), gd, bd, 0, s, p);                        \
      else if (cm == 8) hipLaunchKernelGGL((KERNEL<true, float, 8, W>), gd, bd, 0, s, p);                        \
      else hipLaunchKernelGGL((KERNEL<true, float, 16, W>), gd, bd, 0, s, p);                                    \
    } else if ((d)->dtype == OCT_DT_BF16) {                                                                      \
      if (cm == 2) hipLaunchKernelGGL((KERNEL<false, bf16_t, 2, W>), gd, bd, 0, s, p);                           \
      else if (cm == 4) hipLaunchKernelGGL((KERNEL<false, bf16_t, 4, W>), gd, bd, 0, s, p);                      \
      else if (cm == 8) hipLaunchKernelGGL((KERNEL<false, bf16_t, 8, W>), gd, bd, 0, s, p);                      \
      else hipLaunchKernelGGL((KERNEL<false, bf16_t, 16, W>), gd, bd, 0, s, p);                                  \
    } else {                                                                                                     \
      if (cm == 2) hipLaunchKernelGGL((KERNEL<false, float, 2, W>), gd, bd, 0, s, p);                            \
      else if (cm == 4) hipLaunchKernelGGL((KERNEL<false, float, 4, W>), gd, bd, 0, s, p);                       \
      else if (cm == 8) hipLaunchKernelGGL((KERNEL<false, float, 8, W>), gd, bd, 0, s, p);                       \
      else hipLaunchKernelGGL((KERNEL<false, float, 16, W>), gd, bd, 0, s, p);                                   \
    }                                                                                                            \
  } while (0)

extern "C" int oct_seg_loss_forward(const OctHeadDesc* d, int layout, const void* logits, const int64_t* target,
                                    int64_t* argmax, double* loss_partials, void* stream) {
  int rc = seg_check(d, layout, "oct_seg_loss_forward");
  if (rc) return rc;
  OCT_CHECK(logits, "oct_seg_loss_forward: null pointer (logits)");
  OCT_CHECK(argmax || loss_partials, "oct_seg_loss_forward: null pointer (neither argmax nor loss_partials)");
  OCT_CHECK(!loss_partials || target, "oct_seg_loss_forward: null pointer (loss partials need a target)");
  SegParams p = seg_params(d, logits);
  p.target = target; p.argmax = argmax; p.loss_partials = loss_partials;
  const int grid = oct_seg_loss_blocks(p.npix, d->classes);
  hipStream_t s = as_stream(stream);
  SEG_DISPATCH(seg_fwd_kernel, false, d, layout, grid, s, p);
  return oct_check_launch("seg_loss_fwd");
}

extern "C" int oct_seg_loss_backward(const OctHeadDesc* d, int layout, const void* logits, const int64_t* target,
                                     const float* dice_coef, float w_ce, const float* dloss, void* dlogits,
                                     double* loss_partials, void* stream) {
  int rc = seg_check(d, layout, "oct_seg_loss_backward");
  if (rc) return rc;
  OCT_CHECK(logits && target && dlogits, "oct_seg_loss_backward: null pointer (logits, target and dlogits are required)");
  OCT_CHECK(!(loss_partials && dice_coef), "oct_seg_loss_backward: CE rows come from the backward only without a Dice term");
  SegParams p = seg_params(d, logits);
  p.target = target; p.dice_coef = dice_coef; p.w_ce = w_ce; p.dloss = dloss; p.dlogits = dlogits;
  p.loss_partials = loss_partials;
  p.vec_out = ((uintptr_t)dlogits & 15) == 0;
  const int grid = oct_seg_loss_blocks(p.npix, d->classes);
  hipStream_t s = as_stream(stream);
  SEG_DISPATCH(seg_bwd_kernel, false, d, layout, grid, s, p);
  return oct_check_launch("seg_loss_bwd");
}

// ---- weighted forms: class weights, a pixel weight map, ignore_index (each optional) -------------------------------------
static void seg_weights(SegParams& p, const float* class_weight, const float* pixel_weight, int has_ignore, int64_t ignore_index) {
  p.class_weight = class_weight; p.pixel_weight = pixel_weight;
  p.has_ignore = has_ignore != 0; p.ignore_index = (long long)ignore_index;
}

extern "C" int oct_seg_loss_weight_sum(const OctHeadDesc* d, const int64_t* target, const float* class_weight,
                                       const float* pixel_weight, int has_ignore, int64_t ignore_index, double* partials,
                                       double* wsum, void* stream) {
  int rc = seg_check(d, OCT_SEG_NHWC, "oct_seg_loss_weight_sum");
  if (rc) return rc;
  OCT_CHECK(target && partials && wsum, "oct_seg_loss_weight_sum: null pointer (target, partials and wsum are required)");
  SegParams p = seg_params(d, nullptr);
  p.target = target; p.wsum_partials = partials;
  seg_weights(p, class_weight, pixel_weight, has_ignore, ignore_index);
  const int grid = oct_seg_loss_blocks(p.npix, d->classes);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(seg_wsum_kernel, dim3(grid), dim3(SEG_THREADS), 0, s, p);
  hipLaunchKernelGGL(seg_wsum_reduce_kernel, dim3(1), dim3(64), 0, s, partials, grid, wsum);
  return oct_check_launch("seg_loss_weight_sum");
}

extern "C" int oct_seg_loss_forward_weighted(const OctHeadDesc* d, int layout, const void* logits, const int64_t* target,
                                             const float* class_weight, const float* pixel_weight, int has_ignore,
                                             int64_t ignore_index, double* loss_partials, void* stream) {
  int rc = seg_check(d, layout, "oct_seg_loss_forward_weighted");
  if (rc) return rc;
  OCT_CHECK(logits, "oct_seg_loss_forward_weighted: null pointer (logits)");
  OCT_CHECK(target && loss_partials, "oct_seg_loss_forward_weighted: null pointer (target and loss_partials are required)");
  SegParams p = seg_params(d, logits);
  p.target = target; p.loss_partials = loss_partials;
  seg_weights(p, class_weight, pixel_weight, has_ignore, ignore_index);
  const int grid = oct_seg_loss_blocks(p.npix, d->classes);
  hipStream_t s = as_stream(stream);
  SEG_DISPATCH(seg_fwd_kernel, true, d, layout, grid, s, p);
  return oct_check_launch("seg_loss_fwd_weighted");
}

extern "C" int oct_seg_loss_backward_weighted(const OctHeadDesc* d, int layout, const void* logits, const int64_t* target,
                                              const float* class_weight, const float* pixel_weight, int has_ignore,
                                              int64_t ignore_index, const double* wsum, const float* dice_coef, float w_ce,
                                              const float* dloss, void* dlogits, double* loss_partials, void* stream) {
  int rc = seg_check(d, layout, "oct_seg_loss_backward_weighted");
  if (rc) return rc;
  OCT_CHECK(logits, "oct_seg_loss_backward_weighted: null pointer (logits)");
  OCT_CHECK(target && dlogits && wsum,
            "oct_seg_loss_backward_weighted: null pointer (target, dlogits and wsum are required)");
  OCT_CHECK(!(loss_partials && dice_coef),
            "oct_seg_loss_backward_weighted: CE rows come from the backward only without a Dice term");
  SegParams p = seg_params(d, logits);
  p.target = target; p.dice_coef = dice_coef; p.w_ce = w_ce; p.dloss = dloss; p.dlogits = dlogits;
  p.loss_partials = loss_partials; p.wsum = wsum;
  p.vec_out = ((uintptr_t)dlogits & 15) == 0;
  seg_weights(p, class_weight, pixel_weight, has_ignore, ignore_index);
  const int grid = oct_seg_loss_blocks(p.npix, d->classes);
  hipStream_t s = as_stream(stream);
  SEG_DISPATCH(seg_bwd_kernel, true, d, layout, grid, s, p);
  return oct_check_launch("seg_loss_bwd_weighted");
}

extern "C" int oct_seg_loss_finalize_weighted(const OctHeadDesc* d, const double* loss_partials, int nblocks, float w_ce,
                                              float w_dice, float dice_eps, float* loss_out, float* dice_coef, double* wsum_out,
                                              void* stream) {
  int rc = seg_check(d, OCT_SEG_NHWC, "oct_seg_loss_finalize_weighted");
  if (rc) return rc;
  OCT_CHECK(loss_partials && loss_out && dice_coef, "oct_seg_loss_finalize_weighted: null pointer (rows, loss_out, dice_coef)");
  OCT_CHECK(nblocks > 0, "oct_seg_loss_finalize_weighted: bad row count %d", nblocks);
  hipLaunchKernelGGL(seg_finalize_weighted_kernel, dim3(1), dim3(1024), 0, as_stream(stream), loss_partials, nblocks,
                     d->classes, w_ce, w_dice, dice_eps, loss_out, dice_coef, wsum_out);
  return oct_check_launch("seg_loss_finalize_weighted");
}

// ---- binary / multi-label head: sigmoid BCE + soft Dice on independent channels -------------------------------------------
// Every (pixel, channel) element is its own two-class problem: logit x, target t in {0, 1} from a uint8 mask in NCHW plane
// order (B, C, H, W) whatever the logits' layout -- a lane reads one byte per channel, the lanes of a wave consecutive bytes.
//   valid = !(has_ignore && t == ignore_value);   omega = valid * pixel_weight[pixel]   (one map value for all channels)
//   l     = (1 - t) x + (1 + (pos_weight[c] - 1) t) softplus(-x)     torch's BCEWithLogitsLoss(pos_weight=), stable form
//   BCE   = sum omega l / sum omega;   Dice sums I_c, P_c, Y_c of sigmoid(x) over the valid elements, not weighted
// Same tiling as above (a workgroup owns 256 consecutive pixels, one per lane, every channel of it) and the same rows:
// slot 0 = sum omega l, slot 1 = sum omega, then the Dice sums -- seg_finalize_weighted_kernel finalises them unchanged and its
// dice_coef feeds the backward kernel.  An ignored element enters every sum and the gradient through a select, never through a
// product, so a NaN logit under it cannot leak.  A valid t outside {0, 1} makes l (and the loss) NaN.
// OPTS = false: no pos_weight, no map, no ignore_value -- none of them is read and sum omega is the element count.
struct BceParams {
  SegParams s;   // logits / layout / rows / dice_coef / dloss / dlogits / w_ce (= w_bce) / pixel_weight / wsum / has_ignore
  const unsigned char* target; unsigned char* mask; const float* pos_weight;
  float tau; int ignore_value; int want_dice;
};

// softplus(-x) and sigmoid(x) from one exp(-|x|).  No contraction here or in the two functions below: the forward and the
// backward kernel, in both layouts, must give the same bits for the same element.
__device__ __forceinline__ void bce_terms(float x, float& sp, float& sig) {
#pragma clang fp contract(off)
  const float e = expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  sp = log1pf(e) + fmaxf(-x, 0.f);
  sig = x >= 0.f ? r : e * r;
}

__device__ __forceinline__ float bce_elem(float x, int t, float pw, float sp) {
#pragma clang fp contract(off)
  const float tf = (float)t;
  const float le = (1.f - tf) * x + (1.f + (pw - 1.f) * tf) * sp;
  return t <= 1 ? le : __builtin_nanf("");
}

// g [w_bce k (sig (1 - t + pw t) - pw t) + sig (1 - sig) (A t + B)],  k = omega / sum omega
__device__ __forceinline__ float bce_grad(int t, float pw, float sig, float wk, float a, float b, float g) {
#pragma clang fp contract(off)
  const float tf = (float)t;
  const float pt = pw * tf;
  const float gb = sig * ((1.f - tf) + pt) - pt;
  const float gd = (sig * (1.f - sig)) * (a * tf + b);
  return (wk * gb + gd) * g;
}

// the plane offset of a live lane's pixel: element (img, c, off) of a (B, C, H, W) tensor is at base + c * hw
__device__ __forceinline__ size_t bce_plane_base(const SegParams& s, size_t pix) {
  const size_t img = pix / s.hw;
  return img * (size_t)s.classes * s.hw + (pix - img * s.hw);
}

// mask (may be null): uint8 (B, C, H, W) = x >= tau (a NaN logit gives 0); rows (may be null, need the target)
template <bool NCHW, typename T, int CMAX, bool OPTS>
__global__ void __launch_bounds__(SEG_THREADS) bce_fwd_kernel(const BceParams p) {
  __shared__ __attribute__((aligned(16))) SegStage<T, NCHW ? 1 : CMAX> stage;
  __shared__ double red[SEG_THREADS / 64][OCT_HEAD_LOSS_SLOTS];
  const SegParams& s = p.s;
  const int C = s.classes;
  const bool dice = p.want_dice != 0;
  double ws = 0.0;
  float bce = 0.f, si[CMAX], sp[CMAX], sy[CMAX];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) { si[c] = 0.f; sp[c] = 0.f; sy[c] = 0.f; }
  const size_t ntiles = (s.npix + SEG_THREADS - 1) / SEG_THREADS;
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t p0 = tile * SEG_THREADS, pix = p0 + threadIdx.x;
    const int np = (int)(s.npix - p0 < SEG_THREADS ? s.npix - p0 : SEG_THREADS);
    float l[CMAX];
    seg_load<NCHW, T, CMAX>(s, p0, np, stage.v, l);
    if (threadIdx.x < np) {
      const size_t base = bce_plane_base(s, pix);
      float pm = 1.f;
      if constexpr (OPTS)
        if (s.loss_partials && s.pixel_weight) pm = s.pixel_weight[pix];
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        if (c < C) {
          const float x = l[c];
          if (p.mask) p.mask[base + (size_t)c * s.hw] = x >= p.tau ? 1 : 0;
          if (s.loss_partials) {
            const int t = p.target[base + (size_t)c * s.hw];
            bool valid = true;
            float pw = 1.f;
            if constexpr (OPTS) {
              valid = !(s.has_ignore && t == p.ignore_value);
              if (p.pos_weight) pw = p.pos_weight[c];
            }
            float spl, sig;
            bce_terms(x, spl, sig);
            const float le = bce_elem(x, t, pw, spl);
            if (valid) {   // an ignored element adds exactly nothing, whatever its logit is
              if constexpr (OPTS) { bce = fmaf(pm, le, bce); ws += (double)pm; }
              else { bce += le; ws += 1.0; }
              if (dice) {
                si[c] += t ? sig : 0.f;
                sp[c] += sig;
                sy[c] += (float)t;
              }
            }
          }
        }
      }
    }
    if (!NCHW) __syncthreads();   // the next tile overwrites the stage
  }
  if (s.loss_partials)
    seg_write_row<CMAX, true>(s.loss_partials + (size_t)blockIdx.x * OCT_HEAD_LOSS_SLOTS, bce, si, sp, sy, dice, red, ws);
}

// dlogits in the logits' layout and dtype, exactly 0 for an ignored element; sum omega = *wsum (device double; null: the
// element count); rows (only without a Dice term): slots 0 and 1, so the BCE-only step reads the logits once
template <bool NCHW, typename T, int CMAX, bool OPTS>
__global__ void __launch_bounds__(SEG_THREADS) bce_bwd_kernel(const BceParams p) {
  __shared__ __attribute__((aligned(16))) SegStage<T, NCHW ? 1 : CMAX> stage;
  __shared__ double red[SEG_THREADS / 64][OCT_HEAD_LOSS_SLOTS];
  const SegParams& s = p.s;
  const int C = s.classes;
  const float g = s.dloss ? *s.dloss : 1.f;
  const float inv_n = (float)(1.0 / (s.wsum ? *s.wsum : (double)s.npix * (double)C));
  double ws = 0.0;
  float bce = 0.f;
  T* out = reinterpret_cast<T*>(s.dlogits);
  const size_t ntiles = (s.npix + SEG_THREADS - 1) / SEG_THREADS;
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t p0 = tile * SEG_THREADS, pix = p0 + threadIdx.x;
    const int np = (int)(s.npix - p0 < SEG_THREADS ? s.npix - p0 : SEG_THREADS);
    float l[CMAX];
    seg_load<NCHW, T, CMAX>(s, p0, np, stage.v, l);
    const bool live = threadIdx.x < np;
    if (!NCHW) __syncthreads();   // every lane has read its logits from the stage
    if (live) {
      const size_t base = bce_plane_base(s, pix);
      float pm = 1.f;
      if constexpr (OPTS)
        if (s.pixel_weight) pm = s.pixel_weight[pix];
      const float wk = s.w_ce * (pm * inv_n);
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        if (c < C) {
          const float x = l[c];
          const int t = p.target[base + (size_t)c * s.hw];
          bool valid = true;
          float pw = 1.f;
          if constexpr (OPTS) {
            valid = !(s.has_ignore && t == p.ignore_value);
            if (p.pos_weight) pw = p.pos_weight[c];
          }
          const float a = s.dice_coef ? s.dice_coef[c] : 0.f, b = s.dice_coef ? s.dice_coef[OCT_MAX_CLASSES + c] : 0.f;
          float spl, sig;
          bce_terms(x, spl, sig);
          const float dl = valid ? bce_grad(t, pw, sig, wk, a, b, g) : 0.f;
          if (s.loss_partials && valid) {
            const float le = bce_elem(x, t, pw, spl);
            if constexpr (OPTS) { bce = fmaf(pm, le, bce); ws += (double)pm; }
            else { bce += le; ws += 1.0; }
          }
          if (NCHW) reinterpret_cast<float*>(s.dlogits)[base + (size_t)c * s.hw] = dl;
          else stage.v[threadIdx.x * C + c] = from_f32<T>(dl);
        }
      }
    }
    if (!NCHW) {
      __syncthreads();
      stage_copy<T>(out + p0 * C, stage.v, np * C, s.vec_out);
      __syncthreads();   // the next tile overwrites the stage
    }
  }
  if (s.loss_partials) {
    float z[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) z[c] = 0.f;
    seg_write_row<CMAX, true>(s.loss_partials + (size_t)blockIdx.x * OCT_HEAD_LOSS_SLOTS, bce, z, z, z, false, red, ws);
  }
}

// sum(omega) from the targets and the map alone, in the order the rows' slot 1 is summed: per-lane fp64 sums over the
// channels of each pixel, wave, workgroup, one partial per workgroup.  Without ignore_value the targets are not read.
__global__ void __launch_bounds__(SEG_THREADS) bce_wsum_kernel(const BceParams p) {
  __shared__ double red[SEG_THREADS / 64];
  const SegParams& s = p.s;
  double ws = 0.0;
  const size_t ntiles = (s.npix + SEG_THREADS - 1) / SEG_THREADS;
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t pix = tile * SEG_THREADS + threadIdx.x;
    if (pix < s.npix) {
      const size_t base = bce_plane_base(s, pix);
      const double pm = s.pixel_weight ? (double)s.pixel_weight[pix] : 1.0;
      for (int c = 0; c < s.classes; ++c) {
        const bool valid = !(s.has_ignore && (int)p.target[base + (size_t)c * s.hw] == p.ignore_value);
        if (valid) ws += pm;
      }
    }
  }
  ws = wave_sum(ws);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ws;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    for (int wv = 0; wv < SEG_THREADS / 64; ++wv) a += red[wv];
    s.wsum_partials[blockIdx.x] = a;
  }
}

static int bce_check(const OctHeadDesc* d, int layout, int has_ignore, int ignore_value, const char* who) {
  int rc = seg_check(d, layout, who);
  if (rc) return rc;
  OCT_CHECK(!has_ignore || (ignore_value >= 2 && ignore_value <= 255), "%s: ignore_value %d not in [2,255]", who, ignore_value);
  return OCT_OK;
}

static BceParams bce_params(const OctHeadDesc* d, const void* logits, const uint8_t* target, const float* pos_weight,
                            const float* pixel_weight, int has_ignore, int ignore_value) {
  BceParams p = {};
  p.s = seg_params(d, logits);
  p.s.pixel_weight = pixel_weight; p.s.has_ignore = has_ignore != 0;
  p.target = target; p.pos_weight = pos_weight; p.ignore_value = ignore_value;
  return p;
}

extern "C" int oct_bce_loss_weight_sum(const OctHeadDesc* d, const uint8_t* target, const float* pixel_weight, int has_ignore,
                                       int ignore_value, double* partials, double* wsum, void* stream) {
  int rc = bce_check(d, OCT_SEG_NHWC, has_ignore, ignore_value, "oct_bce_loss_weight_sum");
  if (rc) return rc;
  OCT_CHECK(partials && wsum, "oct_bce_loss_weight_sum: null pointer (partials and wsum are required)");
  OCT_CHECK(target || !has_ignore, "oct_bce_loss_weight_sum: null pointer (ignore_value needs the target)");
  BceParams p = bce_params(d, nullptr, target, nullptr, pixel_weight, has_ignore, ignore_value);
  p.s.wsum_partials = partials;
  const int grid = oct_seg_loss_blocks(p.s.npix, d->classes);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(bce_wsum_kernel, dim3(grid), dim3(SEG_THREADS), 0, s, p);
  hipLaunchKernelGGL(seg_wsum_reduce_kernel, dim3(1), dim3(64), 0, s, partials, grid, wsum);
  return oct_check_launch("bce_loss_weight_sum");
}

extern "C" int oct_bce_loss_forward(const OctHeadDesc* d, int layout, const void* logits, const uint8_t* target,
                                    const float* pos_weight, const float* pixel_weight, int has_ignore, int ignore_value,
                                    int want_dice, float tau, uint8_t* mask, double* loss_partials, void* stream) {
  int rc = bce_check(d, layout, has_ignore, ignore_value, "oct_bce_loss_forward");
  if (rc) return rc;
  OCT_CHECK(logits, "oct_bce_loss_forward: null pointer (logits)");
  OCT_CHECK(mask || loss_partials, "oct_bce_loss_forward: null pointer (neither mask nor loss_partials)");
  OCT_CHECK(!loss_partials || target, "oct_bce_loss_forward: null pointer (loss partials need a target)");
  BceParams p = bce_params(d, logits, target, pos_weight, pixel_weight, has_ignore, ignore_value);
  p.mask = mask; p.tau = tau; p.want_dice = want_dice; p.s.loss_partials = loss_partials;
  const int grid = oct_seg_loss_blocks(p.s.npix, d->classes);
  hipStream_t s = as_stream(stream);
  if (loss_partials && (pos_weight || pixel_weight || has_ignore)) SEG_DISPATCH(bce_fwd_kernel, true, d, layout, grid, s, p);
  else SEG_DISPATCH(bce_fwd_kernel, false, d, layout, grid, s, p);
  return oct_check_launch("bce_loss_fwd");
}

extern "C" int oct_bce_loss_backward(const OctHeadDesc* d, int layout, const void* logits, const uint8_t* target,
                                     const float* pos_weight, const float* pixel_weight, int has_ignore, int ignore_value,
                                     const double* wsum, const float* dice_coef, float w_bce, const float* dloss,
                                     void* dlogits, double* loss_partials, void* stream) {
  int rc = bce_check(d, layout, has_ignore, ignore_value, "oct_bce_loss_backward");
  if (rc) return rc;
  OCT_CHECK(logits && target && dlogits, "oct_bce_loss_backward: null pointer (logits, target and dlogits are required)");
  OCT_CHECK(!(loss_partials && dice_coef), "oct_bce_loss_backward: BCE rows come from the backward only without a Dice term");
  OCT_CHECK(wsum || !(pixel_weight || has_ignore),
            "oct_bce_loss_backward: null pointer (a pixel_weight map or ignore_value needs wsum)");
  BceParams p = bce_params(d, logits, target, pos_weight, pixel_weight, has_ignore, ignore_value);
  p.s.dice_coef = dice_coef; p.s.w_ce = w_bce; p.s.dloss = dloss; p.s.dlogits = dlogits;
  p.s.loss_partials = loss_partials; p.s.wsum = wsum;
  p.s.vec_out = ((uintptr_t)dlogits & 15) == 0;
  const int grid = oct_seg_loss_blocks(p.s.npix, d->classes);
  hipStream_t s = as_stream(stream);
  if (pos_weight || pixel_weight || has_ignore) SEG_DISPATCH(bce_bwd_kernel, true, d, layout, grid, s, p);
  else SEG_DISPATCH(bce_bwd_kernel, false, d, layout, grid, s, p);
  return oct_check_launch("bce_loss_bwd");
}
