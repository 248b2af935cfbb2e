// Paired image / label augmentation (oct_augment_pair): ONE launch per batch warps the image (all channels), the label planes
// and the pixel-weight map of a batch with the SAME per-sample geometry, then runs the intensity stages on the image.
//
// Geometry is fixed point (Q24, evaluated in int64), so a numpy restatement reproduces every index and every bilinear
// fraction bit for bit:
//   SX = a*xo + b*yo + c (+ elastic dx),  SY = d*xo + e*yo + f (+ elastic dy)          output pixel (xo, yo) -> source, Q24
//   floor index ix = SX >> 24, fraction wx = ((SX >> 8) & 0xFFFF) * 2^-16, nearest index (SX + 2^23) >> 24
// The elastic displacement is the integer bilinear blend of four int32 Q24 nodes of a control grid of pitch P = 2^k:
//   (top*(P - ry) + bot*ry) >> 2k,  top = d00*(P - rx) + d01*rx, bot likewise.  No intermediate shift, so the blend may be
//   taken in either order: a thread blends the two node columns of its cell along y once (L, R) and then walks
//   L*P + (R - L)*rx along its run with one 64-bit add per pixel.
// Image and weight-map taps are blended as (1-wy)*((1-wx)*p00 + wx*p01) + wy*((1-wx)*p10 + wx*p11), one fp32 rounding per
// multiply and add (contraction is off for this whole file: __fmul_rn is a plain `*` in this toolchain and would contract).
// Intensity: v*gain + bias -> [gamma: exp2(gamma*log2(clamp01))] -> [noise: v*(1 + s1*z1) + s2*z2] -> clamp -> round.
// Noise: Philox4x32-10, key (seed_lo, seed_hi), counter (pixel >> 1, channel, sample_base + b, step); the even pixel of a
// pair takes words 0,1 and the odd one words 2,3.  Box-Muller on v_log_f32 / v_sqrt_f32 / v_sin_f32 / v_cos_f32 (the last
// two take revolutions, so u2 goes in as it is) -- no precise logf / cosf / powf anywhere.
//
// A thread owns AUG_RUN = 4 consecutive output pixels of one row, starting at a multiple of 4 (8 spilled: 32 tap offsets, 32
// tap values and the run's coordinates do not fit 128 registers).  The coordinates of the run are
// computed once and shared by every image channel, the label planes and the weight map.  Stores are vectors (8 B of bf16, 16 B
// of fp32 / int64, 4 B of mask) where every output base is 16-byte aligned and Wo % 4 == 0 (VEC), element-wise with a bound
// check otherwise.  Source taps are
// gathered straight from global memory (neighbouring lanes share lines; L2 does the rest) with the index CLAMPED into the
// plane before every load, so no coordinate -- however wild the matrix -- reads outside the source.
#pragma clang fp contract(off)
#include "common.h"

#define AUG_RUN 4
#define AUG_THREADS 256
#define AUG_Q 24
#define AUG_MAX_DIM 8192
#define AUG_MAX_PITCH_LOG2 10

struct AugArgs {
  const void* src;
  const void* labels;
  const float* weight;
  const uint32_t* params;   // [batch][OCT_AUG_PARAM_WORDS]
  const int32_t* disp;      // [batch][2][gh][gw] or null
  void* out;
  void* labels_out;
  float* weight_out;
  int batch, cin, hs, ws, ho, wo;
  int label_kind, label_planes;
  int flags, k, gh, gw;
  int runs_per_row;
  long long label_fill;
  float fill;
  uint32_t seed_lo, seed_hi, step, sample_base;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&w)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

__device__ __forceinline__ float aug_val(float v) { return v; }
__device__ __forceinline__ float aug_val(unsigned short v) { return __uint_as_float((unsigned)v << 16); }   // bf16 storage
__device__ __forceinline__ float aug_val(uint8_t v) { return (float)v; }

// floor / nearest index of a Q24 coordinate, clamped to [-2, n] before it leaves 64 bits (anything outside [-1, n) has no tap)
__device__ __forceinline__ int aug_index(long long q, int n) {
  long long i = q >> AUG_Q;
  i = i < -2 ? -2 : i;
  i = i > (long long)n ? (long long)n : i;
  return (int)i;
}

// the four taps of one pixel of one plane; `oob` is what a tap outside the plane reads
template <typename T>
__device__ __forceinline__ float aug_bilinear(const T* __restrict__ plane, int ix, int iy, float wx, float wy, int ws, int hs,
                                              float oob) {
  const bool x0 = ix >= 0 && ix < ws, x1 = ix + 1 >= 0 && ix + 1 < ws;
  const bool y0 = iy >= 0 && iy < hs, y1 = iy + 1 >= 0 && iy + 1 < hs;
  const int cx0 = x0 ? ix : 0, cx1 = x1 ? ix + 1 : 0, cy0 = y0 ? iy : 0, cy1 = y1 ? iy + 1 : 0;   // clamped: every load in bounds
  const float l00 = aug_val(plane[cy0 * ws + cx0]), l01 = aug_val(plane[cy0 * ws + cx1]);
  const float l10 = aug_val(plane[cy1 * ws + cx0]), l11 = aug_val(plane[cy1 * ws + cx1]);
  const float p00 = (x0 && y0) ? l00 : oob, p01 = (x1 && y0) ? l01 : oob;
  const float p10 = (x0 && y1) ? l10 : oob, p11 = (x1 && y1) ? l11 : oob;
  const float ux = 1.0f - wx, uy = 1.0f - wy;   // exact: wx, wy are multiples of 2^-16 in [0, 1)
  const float top = ux * p00 + wx * p01;        // contraction is off: three roundings
  const float bot = ux * p10 + wx * p11;
  return uy * top + wy * bot;
}

template <typename T, int V>
__device__ __forceinline__ void aug_store(T* p, const T (&v)[V], bool vec, int nvalid) {
  if (vec) {
    constexpr int PER = V * sizeof(T) < 16 ? V : 16 / sizeof(T);   // elements per store: the whole run, or 16 bytes of it
    static_assert(V % PER == 0, "a run is a whole number of stores");
#pragma unroll
    for (int q = 0; q < V / PER; ++q) {
      VecT<T, PER> t;
#pragma unroll
      for (int i = 0; i < PER; ++i) t.v[i] = v[q * PER + i];
      *reinterpret_cast<VecT<T, PER>*>(p + q * PER) = t;
    }
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i)
      if (i < nvalid) p[i] = v[i];
  }
}

template <typename OT> __device__ __forceinline__ OT aug_round(float v);
template <> __device__ __forceinline__ float aug_round<float>(float v) { return v; }
template <> __device__ __forceinline__ unsigned short aug_round<unsigned short>(float v) {
  return __builtin_bit_cast(unsigned short, (bf16_t)v);   // round to nearest even
}

template <typename ST, typename OT, bool VEC>
__global__ void __launch_bounds__(AUG_THREADS) __attribute__((amdgpu_waves_per_eu(4, 8))) augment_pair_kernel(const AugArgs p) {
  // a workgroup works on ONE output row of ONE sample: b, yo and with them the parameters, the plane bases and the elastic
  // row blend are wave-uniform (scalar registers), and a tap's address is a uniform base plus a 32-bit lane offset
  const int run = blockIdx.x * blockDim.x + threadIdx.x;
  if (run >= p.runs_per_row) return;
  const int yo = blockIdx.y, b = blockIdx.z;
  const int x0 = run * AUG_RUN;
  const int nvalid = p.wo - x0 < AUG_RUN ? p.wo - x0 : AUG_RUN;   // >= 1

  const uint32_t* pr = p.params + (size_t)b * OCT_AUG_PARAM_WORDS;
  const long long ma = (int)pr[0], mb = (int)pr[1], md = (int)pr[2], me = (int)pr[3];
  const long long mc = (long long)(((unsigned long long)pr[5] << 32) | pr[4]);
  const long long mf = (long long)(((unsigned long long)pr[7] << 32) | pr[6]);
  long long sx = ma * x0 + mb * yo + mc, sy = md * x0 + me * yo + mf;

  // ---- coordinates of the run, shared by every plane -----------------------------------------------------------------------
  int ix[AUG_RUN], iy[AUG_RUN];
  float wx[AUG_RUN], wy[AUG_RUN];
  const bool elastic = (p.flags & OCT_AUG_ELASTIC) != 0;
  const int k = p.k, P = 1 << k, gi = yo >> k, ry = yo & (P - 1);
  const int gi1 = gi + 1 < p.gh ? gi + 1 : p.gh - 1;   // the node past the last row has weight 0: any in-range node does
  const int32_t* dpl = elastic ? p.disp + (size_t)b * 2 * p.gh * p.gw : nullptr;
  long long ex = 0, ey = 0, ddx = 0, ddy = 0;   // L*P + (R - L)*rx of the current cell and its step per pixel
#pragma unroll
  for (int u = 0; u < AUG_RUN; ++u) {
    long long qx = sx, qy = sy;
    if (elastic) {
      const int xo = x0 + u, rx = xo & (P - 1);
      if (u == 0 || rx == 0) {   // a new cell (P >= 4: once per run)
        int gj = xo >> k;
        gj = gj < p.gw ? gj : p.gw - 1;   // only for the pixels past Wo of a partial run
        const int gj1 = gj + 1 < p.gw ? gj + 1 : p.gw - 1;
        const int32_t* d0 = dpl;                            // x displacement plane
        const int32_t* d1 = dpl + (size_t)p.gh * p.gw;      // y displacement plane
        const long long lx = (long long)d0[gi * p.gw + gj] * (P - ry) + (long long)d0[gi1 * p.gw + gj] * ry;
        const long long rxx = (long long)d0[gi * p.gw + gj1] * (P - ry) + (long long)d0[gi1 * p.gw + gj1] * ry;
        const long long ly = (long long)d1[gi * p.gw + gj] * (P - ry) + (long long)d1[gi1 * p.gw + gj] * ry;
        const long long ryy = (long long)d1[gi * p.gw + gj1] * (P - ry) + (long long)d1[gi1 * p.gw + gj1] * ry;
        ddx = rxx - lx; ddy = ryy - ly;
        ex = (lx << k) + ddx * rx; ey = (ly << k) + ddy * rx;
      }
      qx += ex >> (2 * k); qy += ey >> (2 * k);
      ex += ddx; ey += ddy;
    }
    ix[u] = aug_index(qx, p.ws); iy[u] = aug_index(qy, p.hs);
    wx[u] = (float)((unsigned)(qx >> 8) & 0xffffu) * (1.0f / 65536.0f);
    wy[u] = (float)((unsigned)(qy >> 8) & 0xffffu) * (1.0f / 65536.0f);
    sx += ma; sy += md;
  }

  const size_t splane = (size_t)p.hs * p.ws, oplane = (size_t)p.ho * p.wo;
  const size_t orow = (size_t)yo * p.wo + x0;

  // ---- image channels ----------------------------------------------------------------------------------------------------
  if (p.cin > 0) {
    const float gain = __uint_as_float(pr[8]), bias = __uint_as_float(pr[9]), gamma = __uint_as_float(pr[10]);
    const float s_speckle = __uint_as_float(pr[11]), s_add = __uint_as_float(pr[12]);
    const float out_lo = __uint_as_float(pr[13]), out_hi = __uint_as_float(pr[14]);
    const bool do_gamma = (p.flags & OCT_AUG_GAMMA) != 0, do_noise = (p.flags & OCT_AUG_NOISE) != 0;
    const unsigned pix0 = (unsigned)yo * (unsigned)p.wo + (unsigned)x0;   // < 2^26
    for (int c = 0; c < p.cin; ++c) {
      const ST* plane = reinterpret_cast<const ST*>(p.src) + ((size_t)b * p.cin + c) * splane;
      OT res[AUG_RUN];
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int u = 0; u < AUG_RUN; ++u) {
        float v = aug_bilinear<ST>(plane, ix[u], iy[u], wx[u], wy[u], p.ws, p.hs, p.fill);
        v = v * gain + bias;   // two roundings
        if (do_gamma) {
          const float t = fminf(fmaxf(v, 0.0f), 1.0f);
          v = t > 0.0f ? __builtin_amdgcn_exp2f(gamma * __builtin_amdgcn_logf(t)) : 0.0f;
        }
        if (do_noise) {
          const unsigned pix = pix0 + u;
          if (u == 0 || (pix & 1u) == 0u) philox4x32_10(pix >> 1, (uint32_t)c, p.sample_base + (uint32_t)b, p.step, p.seed_lo, p.seed_hi, w);
          const uint32_t wa = (pix & 1u) ? w[2] : w[0], wb = (pix & 1u) ? w[3] : w[1];
          const float u1 = ((float)(wa >> 9) + 0.5f) * (1.0f / 8388608.0f);   // (0, 1), exact
          const float u2 = (float)(wb >> 9) * (1.0f / 8388608.0f);            // [0, 1), exact
          const float r = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));   // sqrt(-2 ln u1)
          const float z1 = r * __builtin_amdgcn_cosf(u2), z2 = r * __builtin_amdgcn_sinf(u2);
          v = v * (1.0f + s_speckle * z1) + s_add * z2;
        }
        v = fminf(fmaxf(v, out_lo), out_hi);
        res[u] = aug_round<OT>(v);
      }
      aug_store<OT, AUG_RUN>(reinterpret_cast<OT*>(p.out) + ((size_t)b * p.cin + c) * oplane + orow, res, VEC, nvalid);
    }
  }

  // ---- pixel-weight map: the same blend, outside taps read 0, no intensity stage ---------------------------------------------
  if (p.weight) {
    const float* plane = p.weight + (size_t)b * splane;
    float res[AUG_RUN];
#pragma unroll
    for (int u = 0; u < AUG_RUN; ++u) res[u] = aug_bilinear<float>(plane, ix[u], iy[u], wx[u], wy[u], p.ws, p.hs, 0.0f);
    aug_store<float, AUG_RUN>(p.weight_out + (size_t)b * oplane + orow, res, VEC, nvalid);
  }

  // ---- label planes: nearest ---------------------------------------------------------------------------------------------
  if (p.label_kind != OCT_AUG_LABEL_NONE) {
    // (SX + 2^23) >> 24 == ix + (bit 23 of SX) == ix + (wx >= 0.5); the clamp of ix to [-2, n] keeps "outside" outside
    bool in[AUG_RUN];
    int off[AUG_RUN];
#pragma unroll
    for (int u = 0; u < AUG_RUN; ++u) {
      const int nx = ix[u] + (wx[u] >= 0.5f ? 1 : 0), ny = iy[u] + (wy[u] >= 0.5f ? 1 : 0);
      in[u] = nx >= 0 && nx < p.ws && ny >= 0 && ny < p.hs;
      off[u] = in[u] ? ny * p.ws + nx : 0;   // clamped: every load in bounds
    }
    if (p.label_kind == OCT_AUG_LABEL_MASK_U8) {
      for (int c = 0; c < p.label_planes; ++c) {
        const uint8_t* plane = reinterpret_cast<const uint8_t*>(p.labels) + ((size_t)b * p.label_planes + c) * splane;
        uint8_t res[AUG_RUN];
#pragma unroll
        for (int u = 0; u < AUG_RUN; ++u) {
          const uint8_t l = plane[off[u]];
          res[u] = in[u] ? l : (uint8_t)p.label_fill;
        }
        uint8_t* o = reinterpret_cast<uint8_t*>(p.labels_out) + ((size_t)b * p.label_planes + c) * oplane + orow;
        aug_store<uint8_t, AUG_RUN>(o, res, VEC, nvalid);
      }
    } else {
      long long res[AUG_RUN];
      if (p.label_kind == OCT_AUG_LABEL_CLASS_U8) {
        const uint8_t* plane = reinterpret_cast<const uint8_t*>(p.labels) + (size_t)b * splane;
#pragma unroll
        for (int u = 0; u < AUG_RUN; ++u) {
          const long long l = plane[off[u]];
          res[u] = in[u] ? l : p.label_fill;
        }
      } else {
        const long long* plane = reinterpret_cast<const long long*>(p.labels) + (size_t)b * splane;
#pragma unroll
        for (int u = 0; u < AUG_RUN; ++u) {
          const long long l = plane[off[u]];
          res[u] = in[u] ? l : p.label_fill;
        }
      }
      aug_store<long long, AUG_RUN>(reinterpret_cast<long long*>(p.labels_out) + (size_t)b * oplane + orow, res, VEC, nvalid);
    }
  }
}

// raw Philox words for given counters: pins the generator bit for bit, nothing else uses it
__global__ void __launch_bounds__(AUG_THREADS) augment_philox_words_kernel(const uint32_t* __restrict__ counters, uint32_t* __restrict__ out,
                                                                           unsigned n, uint32_t k0, uint32_t k1) {
  const unsigned i = blockIdx.x * AUG_THREADS + threadIdx.x;
  if (i >= n) return;
  uint32_t w[4];
  philox4x32_10(counters[4 * (size_t)i], counters[4 * (size_t)i + 1], counters[4 * (size_t)i + 2], counters[4 * (size_t)i + 3], k0, k1, w);
#pragma unroll
  for (int j = 0; j < 4; ++j) out[4 * (size_t)i + j] = w[j];
}

template <typename ST, typename OT>
static void aug_launch(const AugArgs& a, bool vec, hipStream_t s) {
  // whole waves along the row, at most AUG_THREADS lanes; rows on grid.y, samples on grid.z
  const int threads = a.runs_per_row >= AUG_THREADS ? AUG_THREADS : 64 * ((a.runs_per_row + 63) / 64);
  const dim3 grid((a.runs_per_row + threads - 1) / threads, a.ho, a.batch);
  if (vec) hipLaunchKernelGGL((augment_pair_kernel<ST, OT, true>), grid, dim3(threads), 0, s, a);
  else hipLaunchKernelGGL((augment_pair_kernel<ST, OT, false>), grid, dim3(threads), 0, s, a);
}

template <typename ST>
static void aug_launch_out(const AugArgs& a, int out_elem, bool vec, hipStream_t s) {
  if (out_elem == OCT_AUG_F32) aug_launch<ST, float>(a, vec, s);
  else aug_launch<ST, unsigned short>(a, vec, s);
}

static bool aug_aligned(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

extern "C" int oct_augment_pair(const OctAugmentDesc* d, const void* src, const void* labels, const float* weight,
                                const void* params, const int32_t* disp, void* out, void* labels_out, float* weight_out,
                                void* stream) {
  OCT_CHECK(d, "oct_augment_pair: null descriptor");
  OCT_CHECK(d->batch >= 0 && d->cin >= 0 && d->cin <= 65535, "oct_augment_pair: bad batch %d / channels %d", d->batch, d->cin);
  OCT_CHECK(d->hs >= 1 && d->ws >= 1 && d->ho >= 1 && d->wo >= 1, "oct_augment_pair: sizes must be >= 1 (source %d x %d, output %d x %d)",
            d->hs, d->ws, d->ho, d->wo);
  OCT_CHECK(d->hs <= AUG_MAX_DIM && d->ws <= AUG_MAX_DIM && d->ho <= AUG_MAX_DIM && d->wo <= AUG_MAX_DIM,
            "oct_augment_pair: sizes above %d are not supported (source %d x %d, output %d x %d)", AUG_MAX_DIM, d->hs, d->ws, d->ho,
            d->wo);
  OCT_CHECK(d->src_elem >= OCT_AUG_U8 && d->src_elem <= OCT_AUG_F32, "oct_augment_pair: the source is uint8 (0), bf16 (1) or fp32 (2), got %d",
            d->src_elem);
  OCT_CHECK(d->out_elem == OCT_AUG_BF16 || d->out_elem == OCT_AUG_F32, "oct_augment_pair: the output is bf16 (1) or fp32 (2), got %d",
            d->out_elem);
  OCT_CHECK(d->label_kind >= OCT_AUG_LABEL_NONE && d->label_kind <= OCT_AUG_LABEL_MASK_U8, "oct_augment_pair: unknown label kind %d",
            d->label_kind);
  OCT_CHECK(d->label_kind != OCT_AUG_LABEL_MASK_U8 || (d->label_planes >= 1 && d->label_planes <= 65535),
            "oct_augment_pair: a mask needs 1..65535 planes, got %d", d->label_planes);
  OCT_CHECK(d->label_kind != OCT_AUG_LABEL_MASK_U8 || (d->label_fill >= 0 && d->label_fill <= 255),
            "oct_augment_pair: label_fill %lld does not fit a uint8 mask", (long long)d->label_fill);
  OCT_CHECK((d->flags & ~(OCT_AUG_GAMMA | OCT_AUG_NOISE | OCT_AUG_ELASTIC)) == 0, "oct_augment_pair: unknown flags 0x%x", d->flags);
  OCT_CHECK(d->fill == d->fill && d->fill - d->fill == 0.0f, "oct_augment_pair: fill must be finite");
  int k = 0;
  if (d->flags & OCT_AUG_ELASTIC) {
    const int P = d->grid_pitch;
    OCT_CHECK(P >= 1 && (P & (P - 1)) == 0 && P <= (1 << AUG_MAX_PITCH_LOG2),
              "oct_augment_pair: the control-grid pitch must be a power of two in [1, %d], got %d", 1 << AUG_MAX_PITCH_LOG2, P);
    while ((1 << k) < P) ++k;
    OCT_CHECK(disp, "oct_augment_pair: OCT_AUG_ELASTIC without a displacement field");
    OCT_CHECK(aug_aligned(disp, 4), "oct_augment_pair: displacement field not aligned to int32");
  }
  OCT_CHECK(d->batch <= 65535, "oct_augment_pair: at most 65535 samples per call (got %d)", d->batch);
  OCT_CHECK((double)d->batch * (d->cin > 0 ? d->cin : 1) < 2147483648.0 && (double)d->batch * d->label_planes < 2147483648.0,
            "oct_augment_pair: batch * planes must stay below 2^31");
  if (d->batch == 0) return OCT_OK;
  OCT_CHECK(params, "oct_augment_pair: null params");
  OCT_CHECK(aug_aligned(params, 8), "oct_augment_pair: params not aligned to 8 bytes");
  OCT_CHECK(d->cin == 0 || (src && out), "oct_augment_pair: null image");
  OCT_CHECK(d->label_kind == OCT_AUG_LABEL_NONE || (labels && labels_out), "oct_augment_pair: null labels");
  OCT_CHECK((weight == nullptr) == (weight_out == nullptr), "oct_augment_pair: weight and weight_out go together");
  OCT_CHECK(d->cin > 0 || d->label_kind != OCT_AUG_LABEL_NONE || weight, "oct_augment_pair: nothing to do");
  const uintptr_t ssize = d->src_elem == OCT_AUG_F32 ? 4 : d->src_elem == OCT_AUG_BF16 ? 2 : 1;
  const uintptr_t osize = d->out_elem == OCT_AUG_F32 ? 4 : 2;
  OCT_CHECK(aug_aligned(src, ssize) && aug_aligned(out, osize), "oct_augment_pair: image not aligned to its element type");
  OCT_CHECK(aug_aligned(weight, 4) && aug_aligned(weight_out, 4), "oct_augment_pair: weight map not aligned to fp32");
  OCT_CHECK(d->label_kind != OCT_AUG_LABEL_CLASS_I64 || aug_aligned(labels, 8), "oct_augment_pair: int64 class map not aligned");
  OCT_CHECK(d->label_kind == OCT_AUG_LABEL_NONE || d->label_kind == OCT_AUG_LABEL_MASK_U8 || aug_aligned(labels_out, 8),
            "oct_augment_pair: int64 output class map not aligned");

  AugArgs a;
  a.src = d->cin > 0 ? src : nullptr; a.labels = labels; a.weight = weight;
  a.params = reinterpret_cast<const uint32_t*>(params); a.disp = (d->flags & OCT_AUG_ELASTIC) ? disp : nullptr;
  a.out = out; a.labels_out = labels_out; a.weight_out = weight_out;
  a.batch = d->batch; a.cin = d->cin; a.hs = d->hs; a.ws = d->ws; a.ho = d->ho; a.wo = d->wo;
  a.label_kind = d->label_kind; a.label_planes = d->label_kind == OCT_AUG_LABEL_MASK_U8 ? d->label_planes : 1;
  a.flags = d->flags; a.k = k;
  a.gh = ((d->ho - 1 + (1 << k) - 1) >> k) + 1; a.gw = ((d->wo - 1 + (1 << k) - 1) >> k) + 1;
  a.runs_per_row = (d->wo + AUG_RUN - 1) / AUG_RUN;
  a.label_fill = (long long)d->label_fill; a.fill = d->fill;
  a.seed_lo = d->seed_lo; a.seed_hi = d->seed_hi; a.step = d->step; a.sample_base = d->sample_base;
  // vector stores: every run is whole (Wo % 4 == 0) and every output starts on a 16-byte boundary, so every run of every
  // plane row is aligned to its store (4 B mask, 8 B bf16, 16 B fp32 and int64)
  const bool vec = d->wo % AUG_RUN == 0 && (d->cin == 0 || aug_aligned(out, 16)) && aug_aligned(weight_out, 16) &&
                   (d->label_kind == OCT_AUG_LABEL_NONE || aug_aligned(labels_out, 16));
  hipStream_t s = as_stream(stream);
  switch (d->src_elem) {
    case OCT_AUG_U8: aug_launch_out<uint8_t>(a, d->out_elem, vec, s); break;
    case OCT_AUG_BF16: aug_launch_out<unsigned short>(a, d->out_elem, vec, s); break;
    default: aug_launch_out<float>(a, d->out_elem, vec, s); break;
  }
  return oct_check_launch("augment_pair");
}

extern "C" int oct_augment_philox_words(const uint32_t* counters, size_t n, uint32_t key_lo, uint32_t key_hi, uint32_t* out,
                                        void* stream) {
  OCT_CHECK(n < 2147483648ull, "oct_augment_philox_words: n must stay below 2^31");
  if (n == 0) return OCT_OK;
  OCT_CHECK(counters && out, "oct_augment_philox_words: null pointer");
  OCT_CHECK(aug_aligned(counters, 4) && aug_aligned(out, 4), "oct_augment_philox_words: buffers not aligned to uint32");
  const unsigned grid = (unsigned)((n + AUG_THREADS - 1) / AUG_THREADS);
  hipLaunchKernelGGL(augment_philox_words_kernel, dim3(grid), dim3(AUG_THREADS), 0, as_stream(stream), counters, out, (unsigned)n,
                     key_lo, key_hi);
  return oct_check_launch("augment_philox_words");
}
