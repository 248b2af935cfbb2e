// Layer surfaces (oct_surf_extract, oct_surf_paint, oct_surf_error_update): K - 1 ordered boundary rows per A-scan from a class
// map or from scores, by one shortest path per surface with a step limit between neighbouring columns.  The definition, which
// the results reproduce bit for bit, is in include/oct_hip.h; schedule and bytes: DESIGN.md.
//
// A fixed sequence of launches on the caller's stream:
//   cost     one workgroup per (image, SURF_TX columns): phase A, lanes along x, turns SURF_TY rows into the unary bytes
//            u_0..u_{K-1} of every pixel (16 bytes in LDS, [x][y], rows padded by one entry: both phases conflict-free);
//            phase B, lanes along y, one column per wave: d_k from prefix / suffix minima of the bytes, a wave scan per k,
//            the column's carry from LDS, and N[image][k][x][s] written 64 entries = 256 contiguous bytes at a time.
//            max_step < 0: the same kernel keeps, instead of writing N, the least N(x, s) of each column and surface and its
//            smallest s (a wave minimum of (sum, row) keys per chunk), applies the running maximum over k and writes `surfaces`;
//            nothing else runs, no workspace
//   search   one workgroup per (image, k) of T = 256 threads (1024 above 1023 rows), threads over s = r * T + tid.  A(x - 1, .)
//            and A(x, .) are two LDS rows; a step reads the window ascending with a strict <, adds N(x, s), stores the int8
//            offset t - s to P and ends in ONE barrier.  The N entries of the next 8 (1024 threads: 4) columns are in
//            registers before they are used; no divergent branch of the step holds a global access, so the waits on them are
//            counted.  Wave 0 then takes the smallest arg-min of the last row and walks P back: the offsets of the next
//            31 / max_step + 1 columns at the 64 rows around s are loaded at once (the path cannot leave them) and followed
//            with lane reads
//   order    one thread per (image, x): s_k <- max(s_k, s_{k-1})
// Integers throughout, int32 sums (the entry points refuse qmax * h * w >= 2^31); no atomics here.  oct_surf_error_update
// reduces in the wave and adds with 64-bit integer atomics (atomicMax for the largest |e|).
#include "common.h"

#define SURF_U8 0
#define SURF_I64 2
#define SURF_F32 3
#define SURF_BF16 4
#define SURF_TX 32               // columns of a cost tile: 128 contiguous bytes of an fp32 score row
#define SURF_TY 64               // rows of a cost tile: one wave scan
#define SURF_MAX_R 4             // entries of s per search thread: 1024 * 4 = OCT_SURF_MAX_H + 1
#define SURF_EDGE 32             // entries either side of a search row that repeat its first / last entry: OCT_SURF_MAX_STEP
#define SURF_ROW(S) ((S) + 2 * SURF_EDGE + 1)   // a search row in LDS: edge | A(x, 0..h) | edge | one spare entry
#define SURF_ERR_BLOCKS 32       // workgroups per surface of the error update
#define SURF_PAD 255u            // unary byte of a position >= K: above every real u, so no minimum sees it

static_assert(1024 * SURF_MAX_R == OCT_SURF_MAX_H + 1, "the search kernel covers every s of the tallest image");
static_assert(SURF_EDGE >= OCT_SURF_MAX_STEP && 2 * SURF_ROW(OCT_SURF_MAX_H + 1) * 4 <= 64 * 1024,
              "two rows of A within the LDS a kernel gets without opting in");
static_assert(OCT_SURF_MAX_STEP <= 32 && OCT_SURF_MAX_STEP < 128, "the back-walk covers 32 positions each way; offsets fit int8");

struct SurfParams {
  int images, h, w, classes, K, max_step, has_ignore, qmax;
  float scale, qlim;             // qlim = qmax + 1
  long long ignore_index;
  unsigned long long posbits;    // maps: 4 bits per class, its position in `order`
  unsigned long long ordbits;    // 4 bits per position, its class
  unsigned inmask, keepmask;     // bit c: class c is in `order` / in `keep`
  unsigned char chan[16];        // scores: `order`, then every other channel
};

template <int ELEM> struct SurfElem;
template <> struct SurfElem<SURF_U8> { typedef uint8_t T; };
template <> struct SurfElem<SURF_I64> { typedef long long T; };
template <> struct SurfElem<SURF_F32> { typedef float T; };
template <> struct SurfElem<SURF_BF16> { typedef bf16_t T; };

// u_j of scores: floor((m - z) * scale + 0.5), saturated at qmax; every operation rounded on its own
__device__ __forceinline__ unsigned surf_quant(float m, float z, float scale, float qlim, int qmax) {
#pragma clang fp contract(off)   // the product is rounded before the sum: no FMA
  const float diff = z == m ? 0.0f : m - z;
  const float prod = diff * scale;
  const float v = prod + 0.5f;
  return v < qlim ? (unsigned)floorf(v) : (unsigned)qmax;
}

// the unary costs of pixel (img, y, x): u[j], j < K; SURF_PAD for j >= K; all 0 on a free pixel
template <int ELEM, int KM>
__device__ __forceinline__ void surf_unary(const SurfParams& p, const void* __restrict__ in, size_t img, int y, int x, unsigned (&u)[KM]) {
  typedef typename SurfElem<ELEM>::T T;
  const T* src = reinterpret_cast<const T*>(in);
  if constexpr (ELEM == SURF_U8 || ELEM == SURF_I64) {
    const long long v = (long long)src[(img * p.h + y) * (size_t)p.w + x];
    const bool inr = (unsigned long long)v < (unsigned long long)p.classes;
    const unsigned c = inr ? (unsigned)v : 0u;
    const bool is_free = !inr || !((p.inmask >> c) & 1u) || (p.has_ignore && v == p.ignore_index);
    const unsigned pos = (unsigned)(p.posbits >> (4 * c)) & 15u;
#pragma unroll
    for (int j = 0; j < KM; ++j) u[j] = j >= p.K ? SURF_PAD : ((is_free || pos == (unsigned)j) ? 0u : 1u);
  } else {
    const size_t plane = (size_t)p.h * p.w;
    const T* px = src + img * p.classes * plane + (size_t)y * p.w + x;
    float z[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = i < p.classes ? to_f32(px[p.chan[i] * plane]) : 0.0f;
    float m = z[0];
    bool nan = z[0] != z[0];
#pragma unroll
    for (int i = 1; i < 16; ++i)
      if (i < p.classes) {
        m = fmaxf(m, z[i]);
        nan = nan || z[i] != z[i];
      }
#pragma unroll
    for (int j = 0; j < KM; ++j) u[j] = j >= p.K ? SURF_PAD : (nan ? 0u : surf_quant(m, z[j], p.scale, p.qlim, p.qmax));
  }
}

// d[k] = min_{j<k} u_j - min_{j>=k} u_j for k = 1 .. KM-1 (meaningful for k < K)
template <int KM>
__device__ __forceinline__ void surf_split(const unsigned (&u)[KM], int (&d)[KM]) {
  int pm[KM], sm[KM];
  pm[0] = (int)u[0];
#pragma unroll
  for (int j = 1; j < KM; ++j) pm[j] = min(pm[j - 1], (int)u[j]);
  sm[KM - 1] = (int)u[KM - 1];
#pragma unroll
  for (int j = KM - 2; j >= 0; --j) sm[j] = min(sm[j + 1], (int)u[j]);
  d[0] = 0;
#pragma unroll
  for (int k = 1; k < KM; ++k) d[k] = pm[k - 1] - sm[k];
}

// Inclusive scans over the 64 lanes of a wave in DPP steps (no LDS traffic): shifts by 1, 2, 4, 8 inside each row of 16 lanes -- a
// lane without a source takes the identity -- then the last lane of row 0 / 2 into rows 1 / 3 and that of row 1 into rows 2 and 3
template <bool MIN>
__device__ __forceinline__ int surf_wave_scan(int v) {
  constexpr int ident = MIN ? 0x7fffffff : 0;
#define SURF_SCAN_STEP(CTRL, ROWS)                                                         \
  {                                                                                        \
    const int t = __builtin_amdgcn_update_dpp(ident, v, CTRL, ROWS, 0xf, false);           \
    v = MIN ? min(v, t) : v + t;                                                           \
  }
  SURF_SCAN_STEP(0x111, 0xf)   // row_shr:1
  SURF_SCAN_STEP(0x112, 0xf)   // row_shr:2
  SURF_SCAN_STEP(0x114, 0xf)   // row_shr:4
  SURF_SCAN_STEP(0x118, 0xf)   // row_shr:8
  SURF_SCAN_STEP(0x142, 0xa)   // row_bcast:15 into rows 1 and 3
  SURF_SCAN_STEP(0x143, 0xc)   // row_bcast:31 into rows 2 and 3
#undef SURF_SCAN_STEP
  return v;
}

// ---- cost: N[image][k][x][s], or (ARGMIN, max_step < 0) the smallest arg-min of every N(x, .) straight into `surfaces` ------------
template <int ELEM, int KM, bool ARGMIN>
__global__ void __launch_bounds__(256) surf_cost_kernel(const SurfParams p, const void* __restrict__ in, int* __restrict__ N,
                                                        int* __restrict__ surfaces, int xtiles) {
  __shared__ u32x4 tile[SURF_TX * (SURF_TY + 1)];   // [x][y], 16 unary bytes per pixel
  __shared__ int carry[SURF_TX * 16];               // [x][k]: N at the top of the chunk
  __shared__ int bestv[SURF_TX * 16], besta[SURF_TX * 16];   // ARGMIN: the least N(x, s) so far and its smallest s
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t img = blockIdx.x / (unsigned)xtiles;
  const int x0 = (int)(blockIdx.x % (unsigned)xtiles) * SURF_TX;
  const int S = p.h + 1;
  for (int i = tid; i < SURF_TX * 16; i += 256) carry[i] = bestv[i] = besta[i] = 0;   // N(x, 0) = 0
  for (int y0 = 0; y0 < p.h; y0 += SURF_TY) {
    __syncthreads();   // the chunk before has been read (and, the first time, the column state is cleared)
    {                  // phase A: lanes along x
      const int ax = tid & (SURF_TX - 1), ay = tid / SURF_TX;
#pragma unroll 2
      for (int i = 0; i < SURF_TY * SURF_TX / 256; ++i) {
        const int yy = ay + (256 / SURF_TX) * i, y = y0 + yy, x = x0 + ax;
        unsigned u[KM];
        if (y < p.h && x < p.w) {
          surf_unary<ELEM, KM>(p, in, img, y, x, u);
        } else {
#pragma unroll
          for (int j = 0; j < KM; ++j) u[j] = j >= p.K ? SURF_PAD : 0u;   // d = 0 below the image
        }
        u32x4 q = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
#pragma unroll
        for (int wd = 0; wd < KM / 4; ++wd) q[wd] = u[4 * wd] | (u[4 * wd + 1] << 8) | (u[4 * wd + 2] << 16) | (u[4 * wd + 3] << 24);
        tile[ax * (SURF_TY + 1) + yy] = q;
      }
    }
    __syncthreads();
    for (int c = wave; c < SURF_TX; c += 4) {   // phase B: lanes along y, a column per wave
      const int x = x0 + c;
      if (x >= p.w) break;
      const u32x4 q = tile[c * (SURF_TY + 1) + lane];
      unsigned u[KM];
      int d[KM];
#pragma unroll
      for (int j = 0; j < KM; ++j) u[j] = (q[j / 4] >> (8 * (j % 4))) & 255u;
      surf_split<KM>(u, d);
      const int y = y0 + lane;
#pragma unroll
      for (int k = 1; k < KM; ++k)
        if (k < p.K) {
          const int v = surf_wave_scan<false>(d[k]);
          const int top = carry[c * 16 + k];   // v + top = N(x, y + 1): the rows 0..y lie above
          if constexpr (ARGMIN) {
            // |v| <= 255 * 64 < 2^14: (v, lane) as one key whose minimum is the least sum at its smallest row
            const int mine = y < p.h ? ((v + (1 << 14)) << 6) | lane : 0x7fffffff;
            const int key = __builtin_amdgcn_readlane(surf_wave_scan<true>(mine), 63);
            const int least = (key >> 6) - (1 << 14) + top;   // lane 0 is inside the image: the key is real
            if (lane == 0 && least < bestv[c * 16 + k]) {     // strict: ties keep the smallest s
              bestv[c * 16 + k] = least;
              besta[c * 16 + k] = y0 + (key & 63) + 1;
            }
          } else {
            int* row = N + ((img * (p.K - 1) + (k - 1)) * (size_t)p.w + x) * (size_t)S;
            if (y < p.h) row[y + 1] = v + top;
            if (y == 0) row[0] = 0;
          }
          if (lane == 63) carry[c * 16 + k] = v + top;
        }
    }
  }
  if constexpr (ARGMIN) {
    __syncthreads();
    const int x = x0 + tid;
    if (tid < SURF_TX && x < p.w) {
      int run = 0;
      for (int k = 1; k < p.K; ++k) {        // s_k <- max(s_k, s_{k-1})
        run = max(run, besta[tid * 16 + k]);
        surfaces[(img * (p.K - 1) + (k - 1)) * (size_t)p.w + x] = run;
      }
    }
  }
}

// ---- search: the recurrence, the arg-min of the last row and the walk back ---------------------------------------------------------
// blockIdx.x = img * (K - 1) + k; T threads (256; 1024 for images taller than 1023 rows), thread tid owns s = r * T + tid,
// r < R.  DW >= 0: max_step == DW and the window is unrolled; DW < 0: any max_step.  No divergent branch of the step holds a
// global access: a thread past the row works on its last entry and stores nothing, and each LDS row repeats its first and last
// entry max_step times beyond its ends, so that a window is 2 max_step + 1 consecutive entries with no index clamped -- a
// repeated entry equals the edge the ascending scan meets at the clamped t, so the strict < picks the same (value, t).  The
// compiler can then count the loads in flight and need not drain them
template <int R, int DW, int T, int AHEAD>
struct SurfSearch {
  const int* Nc;
  signed char* Pc;
  int *a0, *a1;
  int h, w, delta, tid;
  int n[AHEAD][R];       // N of the columns ahead: slot dd holds column x with (x - 1) % AHEAD == dd

  // A(x, 0) repeated pw times above the row and A(x, h) below it: a window never needs its indices clamped
  __device__ __forceinline__ void edges(int* row, int s, int v, int pw) const {
    if (s == 0)
      for (int j = 1; j <= pw; ++j) row[-j] = v;
    if (s == h)
      for (int j = 1; j <= pw; ++j) row[h + j] = v;
  }

  // one column: A(x, .) into the other LDS row, the offsets into P, slot DD reloaded for column x + AHEAD, one barrier
  template <int DD>
  __device__ __forceinline__ void step(int x) {
    const int S = h + 1;
    const int* cur = (x & 1) ? a0 : a1;
    int* nxt = (x & 1) ? a1 : a0;
    constexpr int G = R < 4 ? R : 4;   // entries whose window reads are in flight together
    const int pw = DW >= 0 ? DW : delta;
#pragma unroll
    for (int g = 0; g < R; g += G) {
      int a[G], bj[G];
#pragma unroll
      for (int i = 0; i < G; ++i) {
        const int* win = cur + (min((g + i) * T + tid, h) - pw);   // the window: win[0 .. 2 pw], the row's edges repeated
        int best = win[0];
        bj[i] = 0;
        if constexpr (DW >= 0) {
          int v[2 * DW + 1];
#pragma unroll
          for (int j = 1; j <= 2 * DW; ++j) v[j] = win[j];
#pragma unroll
          for (int j = 1; j <= 2 * DW; ++j)
            if (v[j] < best) {         // strict, ascending: ties keep the smallest t
              best = v[j];
              bj[i] = j;
            }
        } else {
#pragma unroll 4
          for (int j = 1; j <= 2 * delta; ++j) {
            const int v = win[j];
            if (v < best) {
              best = v;
              bj[i] = j;
            }
          }
        }
        a[i] = n[DD][g + i] + best;
      }
#pragma unroll
      for (int i = 0; i < G; ++i) {
        const int s = (g + i) * T + tid, sc = min(s, h);
        nxt[s < S ? s : S + SURF_EDGE] = a[i];   // a thread past the row writes the spare entry
        if (s == 0 || s == h) edges(nxt, s, a[i], pw);
        // a repeated edge entry stands for the edge itself: t = the window position clamped into the row
        if (s < S) Pc[(size_t)x * S + s] = (signed char)(min(max(s - pw + bj[i], 0), h) - s);
        n[DD][g + i] = Nc[(size_t)min(x + AHEAD, w - 1) * S + sc];   // past the last column: that column again, unused
      }
    }
    __syncthreads();                   // the one barrier of the step: nxt is complete, cur is free to be overwritten
  }

  template <int DD>
  __device__ __forceinline__ void steps(int xb, bool whole) {
    if constexpr (DD < AHEAD) {
      if (whole || xb + DD < w) step<DD>(xb + DD);
      steps<DD + 1>(xb, whole);
    }
  }
};

template <int R, int DW, int T>
__global__ void __launch_bounds__(T) surf_search_kernel(const int* __restrict__ N, signed char* __restrict__ P, int* __restrict__ surfaces,
                                                          int h, int w, int delta) {
  constexpr int AHEAD = T == 256 ? 8 : 4;   // columns of N a thread holds ahead of the step (1024 threads have 128 registers each)
  extern __shared__ int surf_rows[];   // A of the previous and of this column: 2 x SURF_ROW(h + 1)
  const int tid = (int)threadIdx.x, S = h + 1;
  const size_t col = blockIdx.x;
  SurfSearch<R, DW, T, AHEAD> q;
  q.Nc = N + col * (size_t)w * S;
  q.Pc = P + col * (size_t)w * S;
  q.a0 = surf_rows + SURF_EDGE;
  q.a1 = surf_rows + SURF_EDGE + SURF_ROW(S);
  q.h = h; q.w = w; q.delta = delta; q.tid = tid;
  const int* Nc = q.Nc;
  signed char* Pc = q.Pc;
  int* a0 = q.a0;
  int* a1 = q.a1;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int s = r * T + tid;
    if (s < S) {                       // A(0, s) = N(0, s)
      const int v = Nc[s];
      a0[s] = v;
      if (s == 0 || s == h) q.edges(a0, s, v, DW >= 0 ? DW : delta);
    }
  }
#pragma unroll
  for (int dd = 0; dd < AHEAD; ++dd)
#pragma unroll
    for (int r = 0; r < R; ++r) q.n[dd][r] = Nc[(size_t)min(1 + dd, w - 1) * S + min(r * T + tid, h)];
  __syncthreads();
  int xb = 1;
  for (; xb + AHEAD <= w; xb += AHEAD) q.template steps<0>(xb, true);   // whole groups: straight-line code, counted waits
  q.template steps<0>(xb, false);                                         // the last columns, fewer than AHEAD
  if (tid >= 64) return;             // no barrier follows
  // wave 0: the smallest arg-min of A(w - 1, .); P of this workgroup is visible behind the last barrier
  const int* fin = ((w - 1) & 1) ? a1 : a0;
  const int lane = tid;
  int best = 0x7fffffff, bs = S;       // bs = S: no entry yet
  for (int s = lane; s < S; s += 64) {
    const int v = fin[s];
    if (bs == S || v < best) {
      best = v;
      bs = s;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int ov = __shfl_xor(best, o), os = __shfl_xor(bs, o);
    if (os < S && (bs == S || ov < best || (ov == best && os < bs))) {
      best = ov;
      bs = os;
    }
  }
  int* out = surfaces + col * (size_t)w;
  int s = __builtin_amdgcn_readfirstlane(bs);   // the same in every lane: kept scalar
  if (lane == 0) out[w - 1] = s;
  // the walk back, J columns at a time: after j steps the path is within j * delta <= 31 rows of s, so the offsets of column
  // x - j at the 64 rows s - 32 + lane hold the one it needs
  const int J = delta == 0 ? 32 : min(32, 31 / delta + 1);
  for (int x = w - 1; x >= 1; x -= J) {
    const int base = s - 32, cand = base + lane;
    const bool inside = cand >= 0 && cand < S;
    int pj[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) pj[j] = (j < J && x - j >= 1 && inside) ? (int)Pc[(size_t)(x - j) * S + cand] : 0;
    int mine = 0;                      // lane j keeps s(x - 1 - j): one store per batch, none on the walk's critical path
#pragma unroll
    for (int j = 0; j < 32; ++j)
      if (j < J && x - j >= 1) {
        s += __builtin_amdgcn_readlane(pj[j], s - base);   // s - base in [1, 63]
        if (lane == j) mine = s;
      }
    if (lane < min(J, x)) out[x - 1 - lane] = mine;
  }
}

// s_k <- max(s_k, s_{k-1}); one thread per (image, x)
__global__ void __launch_bounds__(256) surf_order_kernel(int* __restrict__ surfaces, size_t columns, int w, int K) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= columns) return;
  const size_t img = i / (unsigned)w;
  const int x = (int)(i % (unsigned)w);
  int* sp = surfaces + img * (K - 1) * (size_t)w + x;
  int run = 0;
  for (int k = 0; k < K - 1; ++k) {
    run = max(run, sp[(size_t)k * w]);
    sp[(size_t)k * w] = run;
  }
}

// ---- paint: out(y, x) = order[#{k : s_k(x) <= y}], or the input class where `keep` lists it ----------------------------------------
// blockIdx.x = (img * ybands + band) * strips + strip; a thread owns one x and SURF_TY rows
template <int ELEM, typename OT>
__global__ void __launch_bounds__(256) surf_paint_kernel(const SurfParams p, const void* in, const int* __restrict__ surfaces,
                                                         OT* out, int strips, int ybands) {
  typedef typename SurfElem<ELEM>::T T;
  const int strip = (int)(blockIdx.x % (unsigned)strips);
  const size_t ib = blockIdx.x / (unsigned)strips;
  const int band = (int)(ib % (unsigned)ybands);
  const size_t img = ib / (unsigned)ybands;
  const int x = strip * 256 + (int)threadIdx.x;
  if (x >= p.w) return;
  int sk[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) sk[k] = k < p.K - 1 ? surfaces[(img * (p.K - 1) + k) * (size_t)p.w + x] : 0x7fffffff;
  const T* src = reinterpret_cast<const T*>(in);
  const size_t plane = (size_t)p.h * p.w;
  const int y1 = min(p.h, (band + 1) * SURF_TY);
  for (int y = band * SURF_TY; y < y1; ++y) {
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 15; ++k) cnt += sk[k] <= y ? 1 : 0;
    long long v = (long long)((p.ordbits >> (4 * cnt)) & 15ull);
    if (p.keepmask) {
      long long cls;
      if constexpr (ELEM == SURF_U8 || ELEM == SURF_I64) {
        cls = (long long)src[img * plane + (size_t)y * p.w + x];
      } else {                         // the arg-max of the package: first maximum, the first NaN beats everything
        const T* px = src + img * p.classes * plane + (size_t)y * p.w + x;
        float bv = to_f32(px[0]);
        int bc = 0;
        for (int c = 1; c < p.classes; ++c) {
          const float l = to_f32(px[c * plane]);
          if (l > bv || (l != l && bv == bv)) {
            bv = l;
            bc = c;
          }
        }
        cls = bc;
      }
      if ((unsigned long long)cls < (unsigned long long)p.classes && ((p.keepmask >> (unsigned)cls) & 1u)) v = cls;
    }
    out[img * plane + (size_t)y * p.w + x] = (OT)v;
  }
}

// Surface rows are expected in [0, OCT_SURF_MAX_H] (what oct_surf_extract writes): the int64 sums are then exact for any
// batch; values the caller made up are not range-checked, and |e| near 2^32 would wrap sum e^2
// ---- position error: count, sum |e|, sum e, sum e^2, max |e| per surface -------------------------------------------------------------
// blockIdx.y = k; the at most SURF_ERR_BLOCKS workgroups of a surface stride over its (image, x) columns: few atomics per address
__global__ void __launch_bounds__(256) surf_error_kernel(const int* __restrict__ target, const int* __restrict__ pred,
                                                         const uint8_t* __restrict__ valid, unsigned long long* __restrict__ state,
                                                         size_t columns, int w, int K) {
  const int k = (int)blockIdx.y;
  long long cnt = 0, sa = 0, se = 0, sq = 0, mx = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < columns; i += (size_t)gridDim.x * 256) {
    if (valid && !valid[i]) continue;
    const size_t img = i / (unsigned)w;
    const size_t o = (img * (K - 1) + k) * (size_t)w + i % (unsigned)w;
    const long long e = (long long)pred[o] - (long long)target[o], ae = e < 0 ? -e : e;
    cnt += 1;
    sa += ae;
    se += e;
    sq += e * e;
    mx = ae > mx ? ae : mx;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o);
    sa += __shfl_xor(sa, o);
    se += __shfl_xor(se, o);
    sq += __shfl_xor(sq, o);
    const long long om = __shfl_xor(mx, o);
    mx = om > mx ? om : mx;
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    unsigned long long* st = state + 5 * k;
    atomicAdd(&st[0], (unsigned long long)cnt);
    atomicAdd(&st[1], (unsigned long long)sa);
    atomicAdd(&st[2], (unsigned long long)se);   // two's complement: the wrapped sum is the signed sum
    atomicAdd(&st[3], (unsigned long long)sq);
    atomicMax(&st[4], (unsigned long long)mx);
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
static inline size_t surf_align(size_t v) { return (v + 255) & ~(size_t)255; }
static inline bool surf_is_map(int elem) { return elem == SURF_U8 || elem == SURF_I64; }

static int surf_check_desc(const OctSurfDesc* d, const char* who) {
  OCT_CHECK(d, "%s: null descriptor", who);
  OCT_CHECK(d->elem == SURF_U8 || d->elem == SURF_I64 || d->elem == SURF_F32 || d->elem == SURF_BF16,
            "%s: the input is a uint8 (0) or int64 (2) map or fp32 (3) or bf16 (4) scores, got %d", who, d->elem);
  OCT_CHECK(d->classes >= 1 && d->classes <= OCT_MAX_CLASSES, "%s: classes must be 1..%d (got %d)", who, OCT_MAX_CLASSES, d->classes);
  OCT_CHECK(d->images >= 0 && d->h >= 1 && d->w >= 1, "%s: bad geometry %d x %d x %d", who, d->images, d->h, d->w);
  OCT_CHECK(d->h <= OCT_SURF_MAX_H, "%s: h must not exceed %d (got %d)", who, OCT_SURF_MAX_H, d->h);
  OCT_CHECK(d->k >= 2 && d->k <= OCT_SURF_MAX_K, "%s: order must name 2..%d classes (got %d)", who, OCT_SURF_MAX_K, d->k);
  OCT_CHECK(d->max_step >= -1 && d->max_step <= OCT_SURF_MAX_STEP, "%s: max_step must be -1 (none) or 0..%d (got %d)", who,
            OCT_SURF_MAX_STEP, d->max_step);
  OCT_CHECK(d->nkeep >= 0 && d->nkeep <= OCT_MAX_CLASSES, "%s: keep names 0..%d classes (got %d)", who, OCT_MAX_CLASSES, d->nkeep);
  int qmax = 1;
  if (!surf_is_map(d->elem)) {
    OCT_CHECK(d->qmax >= 1 && d->qmax <= 255, "%s: qmax must be 1..255 (got %d)", who, d->qmax);
    OCT_CHECK(d->scale > 0.0f && d->scale <= 3.402823466e38f, "%s: scale must be finite and positive", who);
    qmax = d->qmax;
  }
  OCT_CHECK((double)qmax * d->h * d->w < 2147483648.0, "%s: qmax * h * w must stay below 2^31 (int32 path costs), got %d x %d x %d", who,
            qmax, d->h, d->w);
  return OCT_OK;
}

// order: HOST int32 [d->k], distinct classes; keep: HOST int32 [nkeep], disjoint from order (extraction passes none)
static int surf_params(const OctSurfDesc* d, const int32_t* order, const int32_t* keep, int nkeep, SurfParams* p, const char* who) {
  OCT_CHECK(order, "%s: null order", who);
  OCT_CHECK(nkeep == 0 || keep, "%s: null keep list", who);
  *p = SurfParams{};
  p->images = d->images; p->h = d->h; p->w = d->w; p->classes = d->classes; p->K = d->k; p->max_step = d->max_step;
  p->has_ignore = d->has_ignore ? 1 : 0; p->ignore_index = (long long)d->ignore_index;
  const bool map = surf_is_map(d->elem);
  p->qmax = map ? 1 : d->qmax;
  p->scale = map ? 1.0f : d->scale;
  p->qlim = (float)(p->qmax + 1);
  for (int j = 0; j < d->k; ++j) {
    const int c = order[j];
    OCT_CHECK(c >= 0 && c < d->classes, "%s: order[%d] = %d, the input has classes 0..%d", who, j, c, d->classes - 1);
    OCT_CHECK(!((p->inmask >> c) & 1u), "%s: order names class %d twice", who, c);
    p->inmask |= 1u << c;
    p->posbits |= (unsigned long long)j << (4 * c);
    p->ordbits |= (unsigned long long)c << (4 * j);
    p->chan[j] = (unsigned char)c;
  }
  int n = d->k;
  for (int c = 0; c < d->classes; ++c)
    if (!((p->inmask >> c) & 1u)) p->chan[n++] = (unsigned char)c;
  for (int i = 0; i < nkeep; ++i) {
    const int c = keep[i];
    OCT_CHECK(c >= 0 && c < d->classes, "%s: keep[%d] = %d, the input has classes 0..%d", who, i, c, d->classes - 1);
    OCT_CHECK(!((p->inmask >> c) & 1u), "%s: class %d is in both keep and order", who, c);
    p->keepmask |= 1u << c;
  }
  return OCT_OK;
}

static int surf_check_input(const OctSurfDesc* d, const void* in, const char* who) {
  OCT_CHECK(in, "%s: null input", who);
  const unsigned align = d->elem == SURF_I64 ? 7u : d->elem == SURF_F32 ? 3u : d->elem == SURF_BF16 ? 1u : 0u;
  OCT_CHECK(((uintptr_t)in & align) == 0, "%s: the input is not aligned to its element", who);
  return OCT_OK;
}

extern "C" size_t oct_surf_workspace_bytes(const OctSurfDesc* d) {
  if (surf_check_desc(d, "oct_surf_workspace_bytes") != OCT_OK || d->max_step < 0) return 0;
  const size_t cells = (size_t)d->images * (d->k - 1) * d->w * ((size_t)d->h + 1);
  return surf_align(cells * sizeof(int)) + surf_align(cells);   // N int32, P int8
}

// the cost kernel of the input's element and of the narrowest of 4, 8, 16 positions that holds K
#define SURF_COST_ELEM(KM, ARGMIN, ...)                                                           \
  switch (d->elem) {                                                                              \
    case SURF_U8: hipLaunchKernelGGL((surf_cost_kernel<SURF_U8, KM, ARGMIN>), __VA_ARGS__); break;   \
    case SURF_I64: hipLaunchKernelGGL((surf_cost_kernel<SURF_I64, KM, ARGMIN>), __VA_ARGS__); break; \
    case SURF_F32: hipLaunchKernelGGL((surf_cost_kernel<SURF_F32, KM, ARGMIN>), __VA_ARGS__); break; \
    default: hipLaunchKernelGGL((surf_cost_kernel<SURF_BF16, KM, ARGMIN>), __VA_ARGS__); break;      \
  }
#define SURF_COST(ARGMIN, ...)                                      \
  if (d->k <= 4) { SURF_COST_ELEM(4, ARGMIN, __VA_ARGS__) }         \
  else if (d->k <= 8) { SURF_COST_ELEM(8, ARGMIN, __VA_ARGS__) }    \
  else { SURF_COST_ELEM(16, ARGMIN, __VA_ARGS__) }

extern "C" int oct_surf_extract(const OctSurfDesc* d, const int32_t* order, const void* in, int32_t* surfaces, void* workspace,
                                void* stream) {
  const char* who = "oct_surf_extract";
  int rc = surf_check_desc(d, who);
  if (rc != OCT_OK) return rc;
  SurfParams p;
  if ((rc = surf_params(d, order, nullptr, 0, &p, who)) != OCT_OK) return rc;
  if (d->images == 0) return OCT_OK;
  if ((rc = surf_check_input(d, in, who)) != OCT_OK) return rc;
  OCT_CHECK(surfaces && ((uintptr_t)surfaces & 3) == 0, "%s: surfaces is null or not 4-byte aligned", who);
  hipStream_t s = as_stream(stream);
  const dim3 b(256);
  const int xtiles = ceil_div(d->w, SURF_TX);
  const size_t cost_blocks = (size_t)d->images * xtiles;
  OCT_CHECK(cost_blocks < 2147483648ull, "%s: the batch needs more than 2^31 workgroups: pass fewer images per call", who);
  if (d->max_step < 0) {
    SURF_COST(true, dim3((unsigned)cost_blocks), b, 0, s, p, in, nullptr, surfaces, xtiles)
    return oct_check_launch(who);
  }
  OCT_CHECK(workspace && ((uintptr_t)workspace & 15) == 0, "%s: the workspace is null or not 16-byte aligned", who);
  const size_t S = (size_t)d->h + 1, paths = (size_t)d->images * (d->k - 1), cells = paths * d->w * S;
  const size_t columns = (size_t)d->images * d->w;
  OCT_CHECK(paths < 2147483648ull && columns / 256 + 1 < 2147483648ull,
            "%s: the batch needs more than 2^31 workgroups: pass fewer images per call", who);
  int* N = reinterpret_cast<int*>(workspace);
  signed char* P = reinterpret_cast<signed char*>(workspace) + surf_align(cells * sizeof(int));
  SURF_COST(false, dim3((unsigned)cost_blocks), b, 0, s, p, in, N, nullptr, xtiles)
  const int T = S <= 1024 ? 256 : 1024, R = ceil_div((int)S, T);
  const size_t lds = 2 * SURF_ROW(S) * sizeof(int);
#define SURF_SEARCH_R(RR, DW, TT) \
  hipLaunchKernelGGL((surf_search_kernel<RR, DW, TT>), dim3((unsigned)paths), dim3(TT), lds, s, N, P, surfaces, d->h, d->w, d->max_step)
#define SURF_SEARCH(DW)                                \
  if (T == 256 && R <= 1) SURF_SEARCH_R(1, DW, 256);   \
  else if (T == 256 && R <= 2) SURF_SEARCH_R(2, DW, 256); \
  else if (T == 256) SURF_SEARCH_R(4, DW, 256);        \
  else if (R <= 2) SURF_SEARCH_R(2, DW, 1024);         \
  else SURF_SEARCH_R(4, DW, 1024)
  switch (d->max_step) {                   // the small windows unrolled, any other by a loop
    case 0: SURF_SEARCH(0); break;
    case 1: SURF_SEARCH(1); break;
    case 2: SURF_SEARCH(2); break;
    case 3: SURF_SEARCH(3); break;
    default: SURF_SEARCH(-1); break;
  }
#undef SURF_SEARCH
#undef SURF_SEARCH_R
  hipLaunchKernelGGL(surf_order_kernel, dim3((unsigned)((columns + 255) / 256)), b, 0, s, surfaces, columns, d->w, d->k);
  return oct_check_launch(who);
}

extern "C" int oct_surf_paint(const OctSurfDesc* d, const int32_t* order, const int32_t* keep, const void* in, const int32_t* surfaces,
                              void* out, void* stream) {
  const char* who = "oct_surf_paint";
  int rc = surf_check_desc(d, who);
  if (rc != OCT_OK) return rc;
  SurfParams p;
  if ((rc = surf_params(d, order, keep, d->nkeep, &p, who)) != OCT_OK) return rc;
  if (d->images == 0) return OCT_OK;
  if (p.keepmask || surf_is_map(d->elem)) {
    if ((rc = surf_check_input(d, in, who)) != OCT_OK) return rc;
  }
  OCT_CHECK(surfaces && ((uintptr_t)surfaces & 3) == 0, "%s: surfaces is null or not 4-byte aligned", who);
  const bool bytes = d->elem == SURF_U8;
  OCT_CHECK(out && (bytes || ((uintptr_t)out & 7) == 0), "%s: the output is null or not aligned to its element", who);
  const int strips = ceil_div(d->w, 256), ybands = ceil_div(d->h, SURF_TY);
  const size_t blocks = (size_t)d->images * ybands * strips;
  OCT_CHECK(blocks < 2147483648ull, "%s: the batch needs more than 2^31 workgroups: pass fewer images per call", who);
  hipStream_t s = as_stream(stream);
  const dim3 g((unsigned)blocks), b(256);
#define SURF_PAINT(ELEM, OT) hipLaunchKernelGGL((surf_paint_kernel<ELEM, OT>), g, b, 0, s, p, in, surfaces, (OT*)out, strips, ybands)
  switch (d->elem) {
    case SURF_U8: SURF_PAINT(SURF_U8, uint8_t); break;
    case SURF_I64: SURF_PAINT(SURF_I64, long long); break;
    case SURF_F32: SURF_PAINT(SURF_F32, long long); break;
    default: SURF_PAINT(SURF_BF16, long long); break;
  }
#undef SURF_PAINT
  return oct_check_launch(who);
}

extern "C" int oct_surf_error_update(const OctSurfDesc* d, const int32_t* target_surf, const int32_t* pred_surf, const uint8_t* valid,
                                     int64_t* state, void* stream) {
  const char* who = "oct_surf_error_update";
  OCT_CHECK(d, "%s: null descriptor", who);
  OCT_CHECK(d->images >= 0 && d->w >= 1, "%s: bad geometry %d x %d", who, d->images, d->w);
  OCT_CHECK(d->k >= 2 && d->k <= OCT_SURF_MAX_K, "%s: 2..%d ordered classes, K - 1 surfaces (got K = %d)", who, OCT_SURF_MAX_K, d->k);
  OCT_CHECK(state && ((uintptr_t)state & 7) == 0, "%s: the state is null or not 8-byte aligned", who);
  if (d->images == 0) return OCT_OK;
  OCT_CHECK(target_surf && pred_surf && (((uintptr_t)target_surf | (uintptr_t)pred_surf) & 3) == 0,
            "%s: the surfaces are null or not 4-byte aligned", who);
  const size_t columns = (size_t)d->images * d->w, all = (columns + 255) / 256, blocks = all < SURF_ERR_BLOCKS ? all : SURF_ERR_BLOCKS;
  hipLaunchKernelGGL(surf_error_kernel, dim3((unsigned)blocks, (unsigned)(d->k - 1)), dim3(256), 0, as_stream(stream), target_surf,
                     pred_surf, valid, reinterpret_cast<unsigned long long*>(state), columns, d->w, d->k);
  return oct_check_launch(who);
}
