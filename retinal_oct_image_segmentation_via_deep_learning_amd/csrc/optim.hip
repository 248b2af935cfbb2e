// Optimizer kernels over the flat fp32 buffers of optim.FlatParams: Adam / AdamW, the global gradient norm with its clip
// coefficient, and the SGD step of bn.hip with a device-side gradient scale.
//
// All of them are streaming kernels: at most 2048 workgroups of 256 threads walk the buffers with a grid stride, 16 bytes per
// lane on the aligned body.  The vector path needs every pointer 16-byte aligned (FlatParams buffers always are); anything else
// takes the scalar kernels, which evaluate the SAME per-element function, so the two paths give the same bits.  No atomics, no
// synchronisation: the clip coefficient travels from oct_grad_norm to the step through device memory.
//
// Every product that feeds an addition is written as an explicit fmaf or kept in its own statement with no addition behind it,
// so the roundings are exactly those listed at each function whatever the contraction mode (tests/optim_ref.py counts them).
#include "common.h"

#define OPT_THREADS 256
#define OPT_MAX_BLOCKS 2048
#define OPT_CHUNK_SHIFT 6   // one decay-mask byte per 64 floats (optim._ALIGN)

static inline int opt_blocks(size_t items) {
  const size_t b = (items + OPT_THREADS - 1) / OPT_THREADS;
  return (int)(b < OPT_MAX_BLOCKS ? b : OPT_MAX_BLOCKS);
}
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// grad_scale * (*dev_scale): one rounding, the same value in every lane
__device__ __forceinline__ float grad_factor(float gscale, const float* __restrict__ dev_scale) {
  return dev_scale ? gscale * dev_scale[0] : gscale;
}
__device__ __forceinline__ float masked_wd(float wd, const uint8_t* __restrict__ mask, size_t i) {
  return (mask && mask[i >> OPT_CHUNK_SHIFT] == 0) ? 0.f : wd;
}

// ---------------------------------------------------------------------------------------------
// Adam / AdamW (torch.optim.Adam / AdamW, single tensor, no amsgrad)
// ---------------------------------------------------------------------------------------------
struct AdamScalars {
  float b1, omb1, b2, omb2, eps, wd, decay, step_size, isb2;   // omb = 1 - beta, decay = 1 - lr*wd, all rounded once on the host
  int decoupled;
};

// roundings, in order: gs (scalar), g*gs, [coupled: fma(wd,p,.)] | [decoupled: p*decay], omb1*g', fma(b1,m,.), g'*g', omb2*(.),
// fma(b2,v,.), sqrt, fma(.,isb2,eps), the quotient, fma(-step_size,q,p)
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float gs, float wd, const AdamScalars& s) {
  float gr = g * gs;
  float pv = p;
  if (wd != 0.f) {
    if (s.decoupled) pv = pv * s.decay;
    else gr = fmaf(wd, pv, gr);
  }
  const float t1 = s.omb1 * gr;
  const float mn = fmaf(s.b1, m, t1);
  const float g2 = gr * gr;
  const float t2 = s.omb2 * g2;
  const float vn = fmaf(s.b2, v, t2);
  const float den = fmaf(sqrtf(vn), s.isb2, s.eps);
  const float q = mn / den;
  p = fmaf(-s.step_size, q, pv);
  m = mn;
  v = vn;
}

__global__ __launch_bounds__(OPT_THREADS) void adam_vec_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                               float* __restrict__ m, float* __restrict__ v, size_t n,
                                                               AdamScalars s, float gscale, const float* __restrict__ dev_scale,
                                                               const uint8_t* __restrict__ mask) {
  const float gs = grad_factor(gscale, dev_scale);
  const size_t n4 = n >> 2, stride = (size_t)gridDim.x * OPT_THREADS;
  for (size_t i = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += stride) {
    f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 mv = reinterpret_cast<const f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<const f32x4*>(v)[i];
    const float wd = masked_wd(s.wd, mask, i << 2);   // four consecutive floats never straddle a 64-float chunk
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pk = pv[k], mk = mv[k], vk = vv[k];
      adam_elem(pk, gv[k], mk, vk, gs, wd, s);
      pv[k] = pk; mv[k] = mk; vv[k] = vk;
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
  }
  // scalar tail: n % 4 elements
  const size_t t = (n4 << 2) + (size_t)blockIdx.x * OPT_THREADS + threadIdx.x;
  if (t < n) adam_elem(p[t], g[t], m[t], v[t], gs, masked_wd(s.wd, mask, t), s);
}

__global__ __launch_bounds__(OPT_THREADS) void adam_scalar_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                  float* __restrict__ m, float* __restrict__ v, size_t n,
                                                                  AdamScalars s, float gscale,
                                                                  const float* __restrict__ dev_scale,
                                                                  const uint8_t* __restrict__ mask) {
  const float gs = grad_factor(gscale, dev_scale);
  for (size_t i = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * OPT_THREADS)
    adam_elem(p[i], g[i], m[i], v[i], gs, masked_wd(s.wd, mask, i), s);
}

extern "C" int oct_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                             float eps, float weight_decay, int decoupled, float step_size, float inv_sqrt_bc2,
                             float grad_scale, const float* dev_scale, const uint8_t* decay_mask, void* stream) {
  OCT_CHECK(p && g && m && v && n > 0, "oct_adam_step: null buffer or n == 0");
  OCT_CHECK(eps > 0.f, "oct_adam_step: eps must be positive");
  OCT_CHECK(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "oct_adam_step: betas must lie in [0, 1)");
  OCT_CHECK(lr >= 0.f && weight_decay >= 0.f, "oct_adam_step: lr and weight_decay must not be negative");
  OCT_CHECK(step_size >= 0.f && inv_sqrt_bc2 >= 1.f,
            "oct_adam_step: step_size = lr/(1-beta1^t) >= 0 and inv_sqrt_bc2 = 1/sqrt(1-beta2^t) >= 1 expected");
  AdamScalars s;
  s.b1 = beta1; s.omb1 = (float)(1.0 - (double)beta1);
  s.b2 = beta2; s.omb2 = (float)(1.0 - (double)beta2);
  s.eps = eps; s.wd = weight_decay;
  s.decay = (float)(1.0 - (double)lr * (double)weight_decay);
  s.step_size = step_size; s.isb2 = inv_sqrt_bc2;
  s.decoupled = decoupled != 0;
  if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v))
    hipLaunchKernelGGL(adam_vec_kernel, dim3(opt_blocks((n + 3) / 4)), dim3(OPT_THREADS), 0, as_stream(stream), p, g, m, v, n, s,
                       grad_scale, dev_scale, decay_mask);
  else
    hipLaunchKernelGGL(adam_scalar_kernel, dim3(opt_blocks(n)), dim3(OPT_THREADS), 0, as_stream(stream), p, g, m, v, n, s,
                       grad_scale, dev_scale, decay_mask);
  return oct_check_launch("adam_step");
}

// ---------------------------------------------------------------------------------------------
// SGD with a device-side gradient scale: the arithmetic of bn.hip's sgd_kernel, expression for expression
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void sgd_elem(float& p, float g, float* __restrict__ buf, size_t i, float gs, float lr, float momentum,
                                         float wd, int first) {
  float gr = g * gs;
  const float pv = p;
  if (wd != 0.f) gr = fmaf(wd, pv, gr);
  if (momentum != 0.f) {
    const float b = first ? gr : fmaf(momentum, buf[i], gr);
    buf[i] = b;
    gr = b;
  }
  p = pv - lr * gr;
}

__global__ __launch_bounds__(OPT_THREADS) void sgd_vec_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                              float* __restrict__ buf, size_t n, float lr, float momentum,
                                                              float wd, float gscale, int first,
                                                              const float* __restrict__ dev_scale,
                                                              const uint8_t* __restrict__ mask) {
  const float gs = grad_factor(gscale, dev_scale);
  const size_t n4 = n >> 2, stride = (size_t)gridDim.x * OPT_THREADS;
  for (size_t i = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += stride) {
    f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    const float w = masked_wd(wd, mask, i << 2);
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (momentum != 0.f && !first) bv = reinterpret_cast<const f32x4*>(buf)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float gr = gv[k] * gs;
      const float pk = pv[k];
      if (w != 0.f) gr = fmaf(w, pk, gr);
      if (momentum != 0.f) {
        const float b = first ? gr : fmaf(momentum, bv[k], gr);
        bv[k] = b;
        gr = b;
      }
      pv[k] = pk - lr * gr;
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    if (momentum != 0.f) reinterpret_cast<f32x4*>(buf)[i] = bv;
  }
  const size_t t = (n4 << 2) + (size_t)blockIdx.x * OPT_THREADS + threadIdx.x;
  if (t < n) sgd_elem(p[t], g[t], buf, t, gs, lr, momentum, masked_wd(wd, mask, t), first);
}

__global__ __launch_bounds__(OPT_THREADS) void sgd_scalar_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                 float* __restrict__ buf, size_t n, float lr, float momentum,
                                                                 float wd, float gscale, int first,
                                                                 const float* __restrict__ dev_scale,
                                                                 const uint8_t* __restrict__ mask) {
  const float gs = grad_factor(gscale, dev_scale);
  for (size_t i = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * OPT_THREADS)
    sgd_elem(p[i], g[i], buf, i, gs, lr, momentum, masked_wd(wd, mask, i), first);
}

extern "C" int oct_sgd_step_scaled(float* p, const float* g, float* buf, size_t n, float lr, float momentum,
                                   float weight_decay, float grad_scale, int first, const float* dev_scale,
                                   const uint8_t* decay_mask, void* stream) {
  OCT_CHECK(p && g && n > 0, "oct_sgd_step_scaled: bad args");
  OCT_CHECK(momentum == 0.f || buf, "oct_sgd_step_scaled: momentum needs a buffer");
  if (aligned16(p) && aligned16(g) && (momentum == 0.f || aligned16(buf)))
    hipLaunchKernelGGL(sgd_vec_kernel, dim3(opt_blocks((n + 3) / 4)), dim3(OPT_THREADS), 0, as_stream(stream), p, g, buf, n, lr,
                       momentum, weight_decay, grad_scale, first, dev_scale, decay_mask);
  else
    hipLaunchKernelGGL(sgd_scalar_kernel, dim3(opt_blocks(n)), dim3(OPT_THREADS), 0, as_stream(stream), p, g, buf, n, lr,
                       momentum, weight_decay, grad_scale, first, dev_scale, decay_mask);
  return oct_check_launch("sgd_step_scaled");
}

// ---------------------------------------------------------------------------------------------
// Global L2 norm of g * grad_scale and the clip coefficient of torch.nn.utils.clip_grad_norm_
// ---------------------------------------------------------------------------------------------
// The square of an fp32 value is exact in fp64, so only the additions round.  Order: every thread adds its elements in index
// order, the wave butterfly (xor 32, 16, ... 1), then wave 0..3 in order; one fp64 row per workgroup.  Nothing depends on timing.
__device__ __forceinline__ void norm_block_store(double acc, double* __restrict__ rows) {
  __shared__ double wsum[OPT_THREADS / 64];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = wsum[0];
#pragma unroll
    for (int w = 1; w < OPT_THREADS / 64; ++w) t += wsum[w];
    rows[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(OPT_THREADS) void sqsum_vec_kernel(const float* __restrict__ g, size_t n, double* __restrict__ rows) {
  const size_t n4 = n >> 2, stride = (size_t)gridDim.x * OPT_THREADS;
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += stride) {
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc = fma((double)gv[k], (double)gv[k], acc);
  }
  const size_t t = (n4 << 2) + (size_t)blockIdx.x * OPT_THREADS + threadIdx.x;
  if (t < n) acc = fma((double)g[t], (double)g[t], acc);
  norm_block_store(acc, rows);
}

__global__ __launch_bounds__(OPT_THREADS) void sqsum_scalar_kernel(const float* __restrict__ g, size_t n, double* __restrict__ rows) {
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * OPT_THREADS)
    acc = fma((double)g[i], (double)g[i], acc);
  norm_block_store(acc, rows);
}

// one workgroup: thread t adds rows [8t, 8t + 8) in index order (2048 rows at most), then the same wave / workgroup order
__global__ __launch_bounds__(OPT_THREADS) void norm_finalize_kernel(const double* __restrict__ rows, int nrows, float gscale,
                                                                    float max_norm, float* __restrict__ out) {
  __shared__ double wsum[OPT_THREADS / 64];
  constexpr int PER = OPT_MAX_BLOCKS / OPT_THREADS;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int r = threadIdx.x * PER + k;
    if (r < nrows) acc += rows[r];
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = wsum[0];
#pragma unroll
    for (int w = 1; w < OPT_THREADS / 64; ++w) t += wsum[w];
    const double norm = fabs((double)gscale) * sqrt(t);
    double coef = (double)max_norm / (norm + 1e-6);
    coef = coef > 1.0 ? 1.0 : coef;          // a NaN norm compares false and stays NaN, an infinite one gives 0: as torch.clamp
    out[0] = (float)norm;
    out[1] = (float)coef;
  }
}

extern "C" int oct_grad_norm_blocks(size_t n) { return n == 0 ? 0 : opt_blocks((n + 3) / 4); }

extern "C" int oct_grad_norm(const float* g, size_t n, float grad_scale, float max_norm, double* partials, float* out,
                             void* stream) {
  OCT_CHECK(g && partials && out && n > 0, "oct_grad_norm: null buffer or n == 0");
  OCT_CHECK(max_norm > 0.f, "oct_grad_norm: max_norm must be positive");
  const int blocks = oct_grad_norm_blocks(n);
  if (aligned16(g))
    hipLaunchKernelGGL(sqsum_vec_kernel, dim3(blocks), dim3(OPT_THREADS), 0, as_stream(stream), g, n, partials);
  else
    hipLaunchKernelGGL(sqsum_scalar_kernel, dim3(blocks), dim3(OPT_THREADS), 0, as_stream(stream), g, n, partials);
  const int rc = oct_check_launch("grad_norm");
  if (rc != OCT_OK) return rc;
  hipLaunchKernelGGL(norm_finalize_kernel, dim3(1), dim3(OPT_THREADS), 0, as_stream(stream), partials, blocks, grad_scale,
                     max_norm, out);
  return oct_check_launch("grad_norm_finalize");
}
