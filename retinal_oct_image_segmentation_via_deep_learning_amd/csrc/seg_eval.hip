// Streaming segmentation evaluator (oct_seg_eval_update): one launch per validation batch ADDS the C x C confusion matrix and
// the per-layer thickness error |T - P| per A-scan of a (target, prediction) pair to an int64 state that stays on the device.
//
// A workgroup owns whole columns: a strip of 64 (128 for a uint8 / uint8 pair) columns of one image over all h rows, so the
// column counts T - P are complete inside the launch -- no scratch buffer, no second launch.  Consecutive lanes take
// consecutive x (a wave's row load is 128 B of uint8, 512 B of int64, 1 KiB of 8-class bf16 logits); the waves split the rows.
//   * confusion matrix: a per-wave LDS histogram [C*C + 2] (+ ignored, invalid).  Label maps are piecewise constant, so a
//     wave-load usually holds one or two distinct (t, p) keys: equal keys are aggregated across the wave (ballot + popcount,
//     one LDS add per distinct key) for EV_ROUNDS rounds -- a `for` with a fixed cap -- and whatever is left after that
//     (uniformly random maps: up to 64 distinct keys per wave) goes in with plain LDS atomic adds.
//   * thickness: a pixel with t == p adds nothing to T - P, so only disagreeing pixels touch the workgroup's LDS column
//     counters diff[c][x] (+1 at t, -1 at p; lane <-> bank, conflict-free); after the rows, sum_x |diff[c][x]| per class.
//   * flush: one 64-bit atomicAdd per non-zero bin and workgroup (<= 512 workgroups walk the strips).
// A label is range-checked before it indexes anything: the key of an out-of-range pixel is the "invalid" bin.
#include <type_traits>
#include "common.h"

#define EV_MAX_WAVES 16
#define EV_BINS (OCT_MAX_CLASSES * OCT_MAX_CLASSES + 2)   // cm | ignored | invalid
#define EV_ROUNDS 4                                       // aggregated rounds before the plain-atomic fallback (<= 64)
#define EV_MAX_GRID 512

struct EvalParams {
  const void* target;
  const void* pred;
  unsigned long long* state;
  int images, h, w, C;
  int has_ignore;
  long long ignore_index;
  int strips_per_image, nstrips;
  int nq;   // NHWC logits: 16-byte loads per pixel (0: element-wise loads)
};

// add 1 to bin `key` of this wave's histogram for every active lane.  Every lane of the wave calls this together.
__device__ __forceinline__ void ev_count(unsigned* hist, bool active, int key, int lane) {
  unsigned long long rem = __ballot(active);
  for (int r = 0; r < EV_ROUNDS; ++r) {   // bounded by construction
    if (rem == 0ull) break;
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)rem) - 1);
    const int k = __builtin_amdgcn_readlane(key, leader);   // an active lane's key: range-checked by the caller
    const unsigned long long m = __ballot(active && key == k);
    if (lane == leader) atomicAdd(&hist[k], (unsigned)__popcll(m));
    rem &= ~m;
  }
  if ((rem >> lane) & 1ull) atomicAdd(&hist[key], 1u);
}

__device__ __forceinline__ float ev_f32(float v) { return v; }
__device__ __forceinline__ float ev_f32(bf16_t v) { return (float)v; }

// arg-max of oct_seg_loss_forward: first maximum wins, the first NaN beats everything (torch.argmax)
template <int CMAX>
__device__ __forceinline__ int ev_argmax(const float (&l)[CMAX], int C) {
  int best = 0;
  float bv = l[0];
#pragma unroll
  for (int c = 1; c < CMAX; ++c)
    if (c < C && (l[c] > bv || (l[c] != l[c] && bv == bv))) { bv = l[c]; best = c; }
  return best;
}

// prediction of pixel (img, y, x) -- always an in-bounds pixel (the caller clamps), so no load is conditional
template <int PK, int CMAX>
__device__ __forceinline__ long long ev_pred(const EvalParams& p, int img, int y, int x) {
  const size_t pix = ((size_t)img * p.h + y) * p.w + x;
  if constexpr (PK == OCT_EVAL_PRED_U8) {
    return (long long)reinterpret_cast<const uint8_t*>(p.pred)[pix];
  } else if constexpr (PK == OCT_EVAL_PRED_I64) {
    return reinterpret_cast<const long long*>(p.pred)[pix];
  } else if constexpr (PK == OCT_EVAL_PRED_NCHW_F32) {
    const float* base = reinterpret_cast<const float*>(p.pred) + (size_t)img * p.C * p.h * p.w + (size_t)y * p.w + x;
    const size_t plane = (size_t)p.h * p.w;
    float l[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) l[c] = base[(size_t)(c < p.C ? c : p.C - 1) * plane];
    return ev_argmax<CMAX>(l, p.C);
  } else {
    typedef typename std::conditional<PK == OCT_EVAL_PRED_NHWC_BF16, bf16_t, float>::type T;
    constexpr int PER = 16 / sizeof(T), NQ = CMAX / PER;
    const T* base = reinterpret_cast<const T*>(p.pred) + pix * p.C;
    float l[CMAX];
    if (p.nq > 0) {   // 16-byte loads: base 16-byte aligned and C * sizeof(T) a multiple of 16
      typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
      struct alignas(16) Chunk { T v[PER]; };
      const u32x4* q = reinterpret_cast<const u32x4*>(base);
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        const u32x4 raw = q[i < p.nq ? i : p.nq - 1];
        const Chunk ch = __builtin_bit_cast(Chunk, raw);
#pragma unroll
        for (int j = 0; j < PER; ++j) l[i * PER + j] = ev_f32(ch.v[j]);
      }
    } else {
#pragma unroll
      for (int c = 0; c < CMAX; ++c) l[c] = ev_f32(base[c < p.C ? c : p.C - 1]);
    }
    return ev_argmax<CMAX>(l, p.C);
  }
}

template <typename TT, int PK, int CMAX>
__global__ void __launch_bounds__(EV_MAX_WAVES * 64) seg_eval_kernel(const EvalParams p) {
  constexpr int NP = (sizeof(TT) == 1 && PK == OCT_EVAL_PRED_U8) ? 2 : 1;   // pixels per lane and row
  constexpr int SW = 64 * NP;                                                 // strip width
  constexpr int U = (PK == OCT_EVAL_PRED_U8 || PK == OCT_EVAL_PRED_I64) ? 4 : 2;   // rows in flight per wave
  __shared__ unsigned hist[EV_MAX_WAVES][EV_BINS];
  __shared__ int diff[OCT_MAX_CLASSES * SW];
  __shared__ unsigned thick[OCT_MAX_CLASSES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int C = p.C, CC = C * C;
  for (int i = tid; i < nw * EV_BINS; i += blockDim.x) (&hist[0][0])[i] = 0u;
  if (tid < OCT_MAX_CLASSES) thick[tid] = 0u;
  unsigned* myhist = hist[wave];
  const TT* tgt = reinterpret_cast<const TT*>(p.target);

  for (long long strip = blockIdx.x; strip < p.nstrips; strip += gridDim.x) {
    const int img = (int)(strip / p.strips_per_image), x0 = (int)(strip - (long long)img * p.strips_per_image) * SW;
    for (int i = tid; i < C * SW; i += blockDim.x) diff[i] = 0;
    __syncthreads();
    for (int y0 = wave; y0 < p.h; y0 += nw * U) {
      long long t64[U][NP], p64[U][NP];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int y = y0 + u * nw, yc = y < p.h ? y : p.h - 1;
#pragma unroll
        for (int v = 0; v < NP; ++v) {
          const int x = x0 + lane + 64 * v, xc = x < p.w ? x : p.w - 1;   // clamped: every load is in bounds
          t64[u][v] = (long long)tgt[((size_t)img * p.h + yc) * p.w + xc];
          p64[u][v] = ev_pred<PK, CMAX>(p, img, yc, xc);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (y0 + u * nw >= p.h) break;   // wave-uniform
#pragma unroll
        for (int v = 0; v < NP; ++v) {
          const bool active = x0 + lane + 64 * v < p.w;
          const long long t = t64[u][v], q = p64[u][v];
          const bool ignored = p.has_ignore && t == p.ignore_index;
          const bool inrange = (unsigned long long)t < (unsigned long long)C && (unsigned long long)q < (unsigned long long)C;
          const int key = !active ? 0 : ignored ? CC : inrange ? (int)t * C + (int)q : CC + 1;
          ev_count(myhist, active, key, lane);
          if (active && !ignored && inrange && t != q) {
            atomicAdd(&diff[(int)t * SW + lane + 64 * v], 1);
            atomicSub(&diff[(int)q * SW + lane + 64 * v], 1);
          }
        }
      }
    }
    __syncthreads();
    // sum_x |T - P| per class: SW is a multiple of 64, so a wave's 64 entries belong to one class
    for (int i = tid; i < C * SW; i += blockDim.x) {
      const int d = diff[i];
      unsigned a = (unsigned)(d < 0 ? -d : d);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
      if (lane == 0 && a) atomicAdd(&thick[i / SW], a);
    }
    __syncthreads();
  }
  __syncthreads();
  // bins: [0, CC) cm, CC ignored, CC + 1 invalid  ->  state: cm | thick_abs[C] | columns | ignored | invalid | updates
  for (int i = tid; i < CC + 2; i += blockDim.x) {
    unsigned long long s = 0ull;
    for (int wv = 0; wv < nw; ++wv) s += hist[wv][i];
    if (s) atomicAdd(&p.state[i < CC ? i : CC + C + 1 + (i - CC)], s);
  }
  if (tid < C && thick[tid]) atomicAdd(&p.state[CC + tid], (unsigned long long)thick[tid]);
  if (blockIdx.x == 0 && tid == 0) {
    atomicAdd(&p.state[CC + C], (unsigned long long)p.images * (unsigned long long)p.w);
    atomicAdd(&p.state[CC + C + 3], 1ull);
  }
}

template <typename TT, int PK>
static void ev_launch(const EvalParams& p, dim3 g, dim3 b, hipStream_t s) {
  if constexpr (PK == OCT_EVAL_PRED_U8 || PK == OCT_EVAL_PRED_I64) {
    hipLaunchKernelGGL((seg_eval_kernel<TT, PK, 1>), g, b, 0, s, p);
  } else {   // the logits are read in 4 / 8 / 16-channel instantiations, like the loss kernels
    if (p.C <= 4) hipLaunchKernelGGL((seg_eval_kernel<TT, PK, 4>), g, b, 0, s, p);
    else if (p.C <= 8) hipLaunchKernelGGL((seg_eval_kernel<TT, PK, 8>), g, b, 0, s, p);
    else hipLaunchKernelGGL((seg_eval_kernel<TT, PK, 16>), g, b, 0, s, p);
  }
}

extern "C" int oct_seg_eval_update(const OctSegEvalDesc* d, const void* target, const void* pred, int64_t* state, void* stream) {
  OCT_CHECK(d, "oct_seg_eval_update: null descriptor");
  OCT_CHECK(state, "oct_seg_eval_update: null state");
  OCT_CHECK(d->classes >= 1 && d->classes <= OCT_MAX_CLASSES, "oct_seg_eval_update: classes must be 1..%d (got %d)", OCT_MAX_CLASSES,
            d->classes);
  OCT_CHECK(d->images >= 0 && d->h >= 1 && d->w >= 1, "oct_seg_eval_update: bad geometry %d x %d x %d", d->images, d->h, d->w);
  OCT_CHECK((double)d->images * d->h * d->w < 2147483648.0, "oct_seg_eval_update: images * h * w must stay below 2^31");
  OCT_CHECK(d->target_elem == 0 || d->target_elem == 2, "oct_seg_eval_update: target class maps are uint8 (0) or int64 (2), got %d",
            d->target_elem);
  OCT_CHECK(d->pred_kind >= OCT_EVAL_PRED_U8 && d->pred_kind <= OCT_EVAL_PRED_NCHW_F32, "oct_seg_eval_update: bad pred_kind %d",
            d->pred_kind);
  OCT_CHECK(d->images == 0 || (target && pred), "oct_seg_eval_update: null input");
  const bool u8 = d->target_elem == 0;
  static const uintptr_t pred_align[5] = {0, 7, 1, 3, 3};   // element alignment only
  OCT_CHECK(u8 || ((uintptr_t)target & 7) == 0, "oct_seg_eval_update: int64 target not 8-byte aligned");
  OCT_CHECK(((uintptr_t)pred & pred_align[d->pred_kind]) == 0, "oct_seg_eval_update: prediction not aligned to its element type");
  EvalParams p;
  p.target = target; p.pred = pred; p.state = reinterpret_cast<unsigned long long*>(state);
  p.images = d->images; p.h = d->h; p.w = d->w; p.C = d->classes;
  p.has_ignore = d->has_ignore ? 1 : 0; p.ignore_index = (long long)d->ignore_index;
  const int sw = (u8 && d->pred_kind == OCT_EVAL_PRED_U8) ? 128 : 64;
  p.strips_per_image = ceil_div(d->w, sw);
  p.nstrips = d->images * p.strips_per_image;   // <= images * w < 2^31
  p.nq = 0;
  if (d->pred_kind == OCT_EVAL_PRED_NHWC_BF16 || d->pred_kind == OCT_EVAL_PRED_NHWC_F32) {
    const int bytes = d->classes * (d->pred_kind == OCT_EVAL_PRED_NHWC_BF16 ? 2 : 4);
    if (bytes % 16 == 0 && ((uintptr_t)pred & 15) == 0) p.nq = bytes / 16;
  }
  int nw = ceil_div(d->h, 4);   // rows are split over the waves, four in flight each
  if (nw > EV_MAX_WAVES) nw = EV_MAX_WAVES;
  const dim3 g(p.nstrips < 1 ? 1 : (p.nstrips > EV_MAX_GRID ? EV_MAX_GRID : p.nstrips)), b(64 * nw);
  hipStream_t s = as_stream(stream);
#define EV(TT)                                                                              \
  switch (d->pred_kind) {                                                                   \
    case OCT_EVAL_PRED_U8: ev_launch<TT, OCT_EVAL_PRED_U8>(p, g, b, s); break;              \
    case OCT_EVAL_PRED_I64: ev_launch<TT, OCT_EVAL_PRED_I64>(p, g, b, s); break;            \
    case OCT_EVAL_PRED_NHWC_BF16: ev_launch<TT, OCT_EVAL_PRED_NHWC_BF16>(p, g, b, s); break; \
    case OCT_EVAL_PRED_NHWC_F32: ev_launch<TT, OCT_EVAL_PRED_NHWC_F32>(p, g, b, s); break;  \
    default: ev_launch<TT, OCT_EVAL_PRED_NCHW_F32>(p, g, b, s); break;                      \
  }
  if (u8) { EV(uint8_t) } else { EV(long long) }
#undef EV
  return oct_check_launch("seg_eval_update");
}
