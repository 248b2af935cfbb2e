// Score evaluator (oct_score_eval_update): one launch per validation batch ADDS, per channel of a binary / multi-label head,
// the histogram of a 16-bit order-preserving key of every score, split by the element's label, to an int64 state that stays
// on the device.  ROC AUC, average precision and the confusion counts at EVERY threshold follow from it on the host.
//
// The key.  key16(v) of a non-NaN float32 v is the order-preserving code of v rounded toward -inf onto the bf16 grid:
//   u = bits(v), h = u >> 16, low = u & 0xFFFF
//   sign clear:  key = 0x8000 + h
//   sign set:    m = (h & 0x7FFF) + (low != 0), capped at 0x7F80;  key = 0x8000 - m
// -0.0 and +0.0 share key 0x8000; keys lie in [0x0080, 0xFF80] (-inf .. +inf); bin k is the half-open interval
// [g(k), g(k+1)) of the real line, g(k) the bf16 value of code k.  So for a threshold theta ON the bf16 grid
// v >= theta <=> key16(v) >= key16(theta) for every fp32 v, negative theta included (the reason for rounding toward -inf,
// not truncating).  theta = 0 (probability 0.5 on logits) is on the grid.  bf16 and uint8 scores convert to float32 exactly,
// so one key space serves all inputs; fp16 is not taken (its 10 mantissa bits do not survive).
//
// A workgroup owns (channel, half of the key range) and walks tiles of at most SC_CHUNK elements of that channel's planes.
// Its LDS holds 32768 packed counters (label 0 in the low, label 1 in the high 16 bits: 128 KB), so both labels of a key cost
// one LDS add.  Equal keys are aggregated across the wave (ballot + popcount, one LDS add per distinct key) for SC_ROUNDS
// rounds -- a constant field is one add per wave-load -- and what is left (i.i.d. scores: up to 64 distinct keys per wave)
// goes in with plain LDS atomic adds.  Before a tile could take a packed half past 2^16 - 1 the counters are flushed: one
// 64-bit atomicAdd per non-zero half of a non-zero bin; integer atomics only, so two runs give the same bits.  The scores are
// read once per half (the two workgroups of a tile are neighbours in the grid).  nan / ignored / invalid are counted by the
// half-0 workgroups in registers.  Every load is unconditional (the index is clamped into the tile) and the key is clamped
// to 16 bits before it indexes anything.
#include "common.h"

#define SC_THREADS 1024
#define SC_HALF_BINS 32768
#define SC_STEP (4 * SC_THREADS)    // elements per workgroup and loop step: four per thread
#define SC_CHUNK (15 * SC_STEP)     // 61440 < 2^16 elements per tile
#define SC_ROUNDS 4                 // aggregated rounds before the plain-atomic fallback
#define SC_LDS_BYTES (SC_HALF_BINS * 4)
static_assert(SC_CHUNK < 65536, "a tile must fit a packed 16-bit half");
static_assert(SC_LDS_BYTES + 64 <= OCT_LDS_CAP, "score_eval LDS");

struct ScoreParams {
  const uint8_t* target;
  const void* scores;
  unsigned long long* state;
  int hw, C;
  int has_ignore, ignore_value;
  int tpp, ntiles, slots;   // tiles per plane, images * tpp, workgroups per (channel, half)
};

__device__ __forceinline__ unsigned sc_key16(unsigned u) {
  const unsigned h = u >> 16, low = u & 0xffffu;
  unsigned m = (h & 0x7fffu) + (low != 0u ? 1u : 0u);
  m = m > 0x7f80u ? 0x7f80u : m;
  const unsigned key = (u >> 31) ? 0x8000u - m : 0x8000u + h;
  return key > 0xffffu ? 0xffffu : key;   // range clamp: nothing a score can hold leaves the table
}

__device__ __forceinline__ unsigned sc_bits(float v) { return __float_as_uint(v); }
__device__ __forceinline__ unsigned sc_bits(unsigned short v) { return (unsigned)v << 16; }        // bf16 storage
__device__ __forceinline__ unsigned sc_bits(uint8_t v) { return __float_as_uint((float)v); }

// four (score bits, target) pairs of a thread for the step at e0 of a tile of n elements starting at `base`
template <typename ST, bool VEC>
__device__ __forceinline__ void sc_load(const ST* __restrict__ sc, const uint8_t* __restrict__ tg, size_t base, int n, int e0,
                                        int tid, unsigned (&bits)[4], unsigned (&tv)[4]) {
  if constexpr (VEC) {   // n % 4 == 0 and base + everything 4-element aligned (checked by the host)
    int e = e0 + 4 * tid;
    e = e < n - 4 ? e : n - 4;   // clamped: every load is in bounds
    const VecT<ST, 4> s = *reinterpret_cast<const VecT<ST, 4>*>(sc + base + e);
    const VecT<uint8_t, 4> t = *reinterpret_cast<const VecT<uint8_t, 4>*>(tg + base + e);
#pragma unroll
    for (int u = 0; u < 4; ++u) { bits[u] = sc_bits(s.v[u]); tv[u] = t.v[u]; }
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int e = e0 + u * SC_THREADS + tid;
      e = e < n ? e : n - 1;
      bits[u] = sc_bits(sc[base + e]);
      tv[u] = tg[base + e];
    }
  }
}

// add one element per `mine` lane to the packed counter of its bin.  Every lane of the wave calls this together.
__device__ __forceinline__ void sc_count(unsigned* lds, bool mine, unsigned bin, bool pos, int lane) {
  unsigned long long rem = __ballot(mine);
  if (rem == 0ull) return;   // wave-uniform
  for (int r = 0; r < SC_ROUNDS; ++r) {   // bounded by construction
    if (rem == 0ull) break;
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)rem) - 1);
    const unsigned k = (unsigned)__builtin_amdgcn_readlane((int)bin, leader);   // a `mine` lane's bin: < SC_HALF_BINS
    const bool same = mine && bin == k;
    const unsigned long long m = __ballot(same), mp = __ballot(same && pos);
    const unsigned np = (unsigned)__popcll(mp), nn = (unsigned)__popcll(m) - np;
    if (lane == leader) atomicAdd(&lds[k], nn + (np << 16));
    rem &= ~m;
  }
  if ((rem >> lane) & 1ull) atomicAdd(&lds[bin], pos ? 0x10000u : 1u);
}

// LDS counters -> state, and zero them.  Called by the whole workgroup.
__device__ __forceinline__ void sc_flush(unsigned* lds, unsigned long long* hist, int tid) {
  __syncthreads();
  u32x4* l4 = reinterpret_cast<u32x4*>(lds);
  for (int i = tid; i < SC_HALF_BINS / 4; i += SC_THREADS) {
    const u32x4 v = l4[i];
    if ((v[0] | v[1] | v[2] | v[3]) == 0u) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned lo = v[j] & 0xffffu, hi = v[j] >> 16;
      if (lo) atomicAdd(&hist[4 * i + j], (unsigned long long)lo);
      if (hi) atomicAdd(&hist[65536 + 4 * i + j], (unsigned long long)hi);
    }
    l4[i] = u32x4{0u, 0u, 0u, 0u};
  }
  __syncthreads();
}

template <typename ST, bool VEC>
__global__ void __launch_bounds__(SC_THREADS) score_eval_kernel(const ScoreParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned sc_lds[];
  __shared__ unsigned spec[3];
  const int tid = threadIdx.x, lane = tid & 63;
  const int half = blockIdx.x & 1, c = (blockIdx.x >> 1) % p.C, slot = (blockIdx.x >> 1) / p.C;
  for (int i = tid; i < SC_HALF_BINS; i += SC_THREADS) sc_lds[i] = 0u;
  if (tid < 3) spec[tid] = 0u;
  __syncthreads();
  const ST* sc = reinterpret_cast<const ST*>(p.scores);
  unsigned long long* hist = p.state + (size_t)c * 131072 + (size_t)half * SC_HALF_BINS;   // [label][key] of this half
  unsigned n_nan = 0u, n_ign = 0u, n_inv = 0u;
  int pending = 0;   // elements counted since the last flush: a packed half holds at most this

  for (int j = slot; j < p.ntiles; j += p.slots) {
    const int img = j / p.tpp, start = (j - img * p.tpp) * SC_CHUNK;
    const int n = p.hw - start < SC_CHUNK ? p.hw - start : SC_CHUNK;
    const size_t base = ((size_t)img * p.C + c) * (size_t)p.hw + start;
    if (pending + n > 65535) { sc_flush(sc_lds, hist, tid); pending = 0; }
    pending += n;
    unsigned bits[4], tv[4];
    sc_load<ST, VEC>(sc, p.target, base, n, 0, tid, bits, tv);
    for (int e0 = 0; e0 < n; e0 += SC_STEP) {
      unsigned nbits[4], ntv[4];
      sc_load<ST, VEC>(sc, p.target, base, n, e0 + SC_STEP, tid, nbits, ntv);   // next step, clamped into the tile
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = VEC ? e0 + 4 * tid + u : e0 + u * SC_THREADS + tid;
        const bool active = e < n;
        const unsigned t = tv[u];
        const bool ignored = p.has_ignore && t == (unsigned)p.ignore_value;
        const bool invalid = !ignored && t > 1u;
        const bool isnan = (bits[u] & 0x7fffffffu) > 0x7f800000u;
        const bool counted = active && !ignored && !invalid;
        n_ign += (active && ignored) ? 1u : 0u;
        n_inv += (active && invalid) ? 1u : 0u;
        n_nan += (counted && isnan) ? 1u : 0u;
        const unsigned key = sc_key16(bits[u]);
        sc_count(sc_lds, counted && !isnan && (int)(key >> 15) == half, key & (SC_HALF_BINS - 1), t == 1u, lane);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) { bits[u] = nbits[u]; tv[u] = ntv[u]; }
    }
  }
  if (pending > 0) sc_flush(sc_lds, hist, tid);
  // nan | ignored | invalid of this channel: the half-0 workgroups saw every element once
  if (half == 0) {
    unsigned v[3] = {n_nan, n_ign, n_inv};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
      if (lane == 0 && v[k]) atomicAdd(&spec[k], v[k]);
    }
  }
  __syncthreads();
  unsigned long long* tail = p.state + (size_t)p.C * 131072;
  if (half == 0 && tid < 3 && spec[tid]) atomicAdd(&tail[tid * p.C + c], (unsigned long long)spec[tid]);
  if (blockIdx.x == 0 && tid == 0) atomicAdd(&tail[3 * p.C], 1ull);
}

template <typename ST>
static int sc_launch(const ScoreParams& p, bool vec, int grid, hipStream_t s) {
  const void* k = vec ? (const void*)score_eval_kernel<ST, true> : (const void*)score_eval_kernel<ST, false>;
  const int rc = oct_lds_optin(k, SC_LDS_BYTES);   // per (device, kernel); its return code is the launch's
  if (rc != OCT_OK) return rc;
  if (vec) hipLaunchKernelGGL((score_eval_kernel<ST, true>), dim3(grid), dim3(SC_THREADS), SC_LDS_BYTES, s, p);
  else hipLaunchKernelGGL((score_eval_kernel<ST, false>), dim3(grid), dim3(SC_THREADS), SC_LDS_BYTES, s, p);
  return oct_check_launch("score_eval_update");
}

extern "C" size_t oct_score_eval_state_elems(int channels) {
  if (channels < 1 || channels > OCT_MAX_CLASSES) return 0;
  return (size_t)channels * (2 * 65536 + 3) + 1;
}

extern "C" int oct_score_eval_update(const OctScoreEvalDesc* d, const uint8_t* target, const void* scores, int64_t* state,
                                     void* stream) {
  OCT_CHECK(d, "oct_score_eval_update: null descriptor");
  OCT_CHECK(state, "oct_score_eval_update: null state");
  OCT_CHECK(d->channels >= 1 && d->channels <= OCT_MAX_CLASSES, "oct_score_eval_update: channels must be 1..%d (got %d)",
            OCT_MAX_CLASSES, d->channels);
  OCT_CHECK(d->images >= 0 && d->h >= 1 && d->w >= 1, "oct_score_eval_update: bad geometry %d x %d x %d", d->images, d->h, d->w);
  OCT_CHECK((double)d->h * d->w < 2147483648.0 && (double)d->images * d->channels * d->h * d->w < 2147483648.0,
            "oct_score_eval_update: h * w and images * channels * h * w must stay below 2^31");
  OCT_CHECK(d->score_elem >= OCT_SCORE_F32 && d->score_elem <= OCT_SCORE_U8,
            "oct_score_eval_update: scores are fp32 (0), bf16 (1) or uint8 (2), got %d", d->score_elem);
  OCT_CHECK(!d->has_ignore || (d->ignore_value >= 2 && d->ignore_value <= 255),
            "oct_score_eval_update: ignore_value %d is not in [2, 255]", d->ignore_value);
  OCT_CHECK(d->images == 0 || (target && scores), "oct_score_eval_update: null input");
  const int esize = d->score_elem == OCT_SCORE_F32 ? 4 : d->score_elem == OCT_SCORE_BF16 ? 2 : 1;
  OCT_CHECK(((uintptr_t)scores & (uintptr_t)(esize - 1)) == 0, "oct_score_eval_update: scores not aligned to their element type");
  ScoreParams p;
  p.target = target; p.scores = scores; p.state = reinterpret_cast<unsigned long long*>(state);
  p.hw = d->h * d->w; p.C = d->channels;
  p.has_ignore = d->has_ignore ? 1 : 0; p.ignore_value = d->ignore_value;
  p.tpp = ceil_div(p.hw, SC_CHUNK);
  p.ntiles = d->images * p.tpp;   // <= images * h * w < 2^31
  int slots = 512 / p.C;          // about 1024 workgroups: every one flushes per tile anyway, so more only balance better
  if (slots > p.ntiles) slots = p.ntiles;
  if (slots < 1) slots = 1;
  p.slots = slots;
  const int grid = p.ntiles == 0 ? 1 : 2 * p.C * slots;   // images == 0: one workgroup that only counts the update
  // four elements per load where every tile starts on a 4-element boundary of both buffers
  const bool vec = p.hw % 4 == 0 && ((uintptr_t)scores & (uintptr_t)(4 * esize - 1)) == 0 && ((uintptr_t)target & 3) == 0;
  hipStream_t s = as_stream(stream);
  switch (d->score_elem) {
    case OCT_SCORE_F32: return sc_launch<float>(p, vec, grid, s);
    case OCT_SCORE_BF16: return sc_launch<unsigned short>(p, vec, grid, s);
    default: return sc_launch<uint8_t>(p, vec, grid, s);
  }
}
