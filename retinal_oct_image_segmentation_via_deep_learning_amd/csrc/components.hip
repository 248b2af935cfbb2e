// Connected components (oct_cc_label, oct_cc_filter, oct_lesion_eval_update): multi-valued labelling of class maps, a cleanup
// filter on the components and lesion-wise detection counts.  Contract: include/oct_hip.h; argument: DESIGN.md.
//
// A pixel's parent is the y*w + x of a pixel of its own component that is not larger than itself; a root is its own parent, so
// the root of a component is its smallest index.  `roots` is the parent array until the last launch:
//   local    one workgroup per CC_TH x CC_TW tile, one wave per row: the runs of a row come from one ballot (parent = the run's
//            first pixel); the runs of adjacent rows are united in LDS (atomicMin, a run pair is united once); each run adds its
//            length and its border bit to the tile-local root's LDS counter.  Writes the classes as bytes, every pixel's parent
//            (the tile-local root as an image index) and, at the tile-local roots, the counter into `info`.
//   border   one thread per pixel of a tile's first row or first column unites it with its neighbours in the adjacent tile (the
//            diagonals too with connectivity 8), a pair of runs along an edge once.  The only launch in which workgroups write
//            what others read: every write is an agent-scope atomicMin whose return value decides, every read of a parent a
//            relaxed agent-scope atomic load.
//   flatten  every pixel walks to its root and stores it; a tile-local root that is not the root adds its counter to the root's
//            (integer atomicAdd of the area, atomicOr of the border bit) and clears its own.
// No workgroup waits on another.  Parents only decrease and stay inside the component, so a stale parent is still an ancestor,
// a walk strictly descends and ends, and a link that lost a race is seen in the atomic's return value and taken up from there.
#include "common.h"

#define CC_TH 32
#define CC_TW 64                 // one wave per row: the run structure of a row is one ballot
#define CC_TILE (CC_TH * CC_TW)
#define CC_ROWS_PER_WAVE (CC_TH / 4)
#define CC_NOCLASS 0xFFu
#define CC_IGNORED 0xFEu
#define CC_MAX_DIM 16384
#define CC_BORDER (1 << OCT_CC_BORDER_BIT)
#define CC_AREA_MASK (CC_BORDER - 1)

static_assert(CC_TW == 64 && CC_TH % 4 == 0, "a 256-thread workgroup: four waves, one row of 64 pixels per wave step");

struct CcWs {   // byte offsets into the workspace
  size_t lab[2], roots[2], info[2], inter[2], best, total;
};

static inline size_t cc_align(size_t v) { return (v + 255) & ~(size_t)255; }

static void cc_layout(const OctCcDesc* d, int op, CcWs* ws) {
  const size_t N = (size_t)d->images * d->h * d->w;
  size_t o = 0;
  *ws = CcWs{};
  ws->lab[0] = o; o += cc_align(N);
  if (op == OCT_CC_OP_FILTER) { ws->best = o; o += cc_align(8 * (size_t)d->images * d->classes); }
  if (op == OCT_CC_OP_LESION) {
    ws->lab[1] = o; o += cc_align(N);
    for (int m = 0; m < 2; ++m) {
      ws->roots[m] = o; o += cc_align(4 * N);
      ws->info[m] = o;  o += cc_align(4 * N);
      ws->inter[m] = o; o += cc_align(4 * N);
    }
  }
  ws->total = o;
}

static int cc_check_desc(const OctCcDesc* d, const char* who) {
  OCT_CHECK(d, "%s: null descriptor", who);
  OCT_CHECK(d->classes >= 1 && d->classes <= OCT_MAX_CLASSES, "%s: classes must be 1..%d (got %d)", who, OCT_MAX_CLASSES, d->classes);
  OCT_CHECK(d->images >= 0 && d->h >= 1 && d->w >= 1, "%s: bad geometry %d x %d x %d", who, d->images, d->h, d->w);
  OCT_CHECK(d->h <= CC_MAX_DIM && d->w <= CC_MAX_DIM, "%s: h and w must not exceed %d (got %d x %d)", who, CC_MAX_DIM, d->h, d->w);
  OCT_CHECK((double)d->images * d->h * d->w < 2147483648.0, "%s: images * h * w must stay below 2^31", who);
  OCT_CHECK(d->map_elem == 0 || d->map_elem == 2, "%s: class maps are uint8 (0) or int64 (2), got %d", who, d->map_elem);
  OCT_CHECK(d->pred_elem == 0 || d->pred_elem == 2, "%s: predicted class maps are uint8 (0) or int64 (2), got %d", who, d->pred_elem);
  OCT_CHECK(d->connectivity == 4 || d->connectivity == 8, "%s: connectivity must be 4 or 8 (got %d)", who, d->connectivity);
  OCT_CHECK(d->op >= OCT_CC_OP_LABEL && d->op <= OCT_CC_OP_LESION, "%s: unknown op %d", who, d->op);
  OCT_CHECK(d->overlap_den >= 1 && d->overlap_num >= 0 && d->overlap_num <= d->overlap_den,
            "%s: the minimum overlap must be a fraction in [0, 1] with a positive denominator (got %d / %d)", who, d->overlap_num,
            d->overlap_den);
  return OCT_OK;
}

// ---- union-find ------------------------------------------------------------------------------------------------------------
// LDS, one workgroup: the same protocol as the global one below, at workgroup scope
__device__ __forceinline__ int cc_lfind(int* P, int x) {
  for (;;) {
    const int p = __hip_atomic_load(&P[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;                                             // p < x: strictly descending
  }
}

__device__ __forceinline__ void cc_lunion(int* P, int a, int b) {
  for (;;) {
    a = cc_lfind(P, a); b = cc_lfind(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }      // a > b: the larger root goes under the smaller
    const int old = __hip_atomic_fetch_min(&P[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == a) return;                              // a was a root at the atomic: linked
    a = old;                                           // a had been linked to old meanwhile: go on with (old, b)
  }
}

// global: a parent another workgroup may write is read with a relaxed agent-scope atomic load.  A stale value is an earlier
// parent of x: larger than the current one, still in the component and still below x.
__device__ __forceinline__ int cc_gfind(int* P, int x) {
  for (;;) {
    const int p = __hip_atomic_load(&P[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
}

// max(a, b) strictly decreases from one round to the next: at most max(a, b) rounds, no waiting
__device__ __forceinline__ void cc_gunion(int* P, int a, int b) {
  for (;;) {
    a = cc_gfind(P, a); b = cc_gfind(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(&P[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;                              // the atomic found a root and linked it
    a = old;                                           // it found a's newer parent (P[a] = min(old, b) now): unite that with b
  }
}

// ---- local -------------------------------------------------------------------------------------------------------------------
// the class of a pixel as a byte; `ign` is the map whose ignore_index puts the pixel outside (the map itself, or the target)
template <typename T, typename U>
__device__ __forceinline__ unsigned cc_class(const T* map, const U* ign, size_t i, int C, int has_ignore, long long ignore_index) {
  const long long v = (long long)map[i];
  if (has_ignore && (long long)ign[i] == ignore_index) return CC_IGNORED;
  return (unsigned long long)v < (unsigned long long)C ? (unsigned)v : CC_NOCLASS;
}

template <typename T, typename U>
__global__ void __launch_bounds__(256) cc_local_kernel(const T* __restrict__ map, const U* __restrict__ ign, uint8_t* __restrict__ lab,
                                                       int* __restrict__ roots, int* __restrict__ info, int h, int w, int C, int conn8,
                                                       int has_ignore, long long ignore_index, int ntx, int nty) {
  __shared__ int s_par[CC_TILE];
  __shared__ int s_cnt[CC_TILE];
  __shared__ uint8_t s_lab[CC_TILE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int tx = (int)(blockIdx.x % (unsigned)ntx);
  const int ty = (int)((blockIdx.x / (unsigned)ntx) % (unsigned)nty);
  const size_t img = blockIdx.x / ((unsigned)ntx * (unsigned)nty);
  const int x0 = tx * CC_TW, y0 = ty * CC_TH;
  const int gx = x0 + lane;
  const size_t base = img * (size_t)h * w;
  unsigned long long starts[CC_ROWS_PER_WAVE];         // per row of this wave: the lanes that begin a run (wave-uniform)
  unsigned mine[CC_ROWS_PER_WAVE];

  // rows wv, wv + 4, ...: classes, runs, parent = first pixel of the run
#pragma unroll
  for (int k = 0; k < CC_ROWS_PER_WAVE; ++k) {
    const int ly = wv + 4 * k, gy = y0 + ly;
    const bool in = gy < h && gx < w;
    const unsigned c = in ? cc_class(map, ign, base + (size_t)gy * w + gx, C, has_ignore, ignore_index) : CC_NOCLASS;
    const unsigned left = (unsigned)__shfl_up((int)c, 1);
    const bool start = lane == 0 || left != c;
    const unsigned long long st = __ballot(start);
    const int first = 63 - __builtin_clzll(st & (~0ull >> (63 - lane)));   // bit 0 is always set
    const int i = ly * CC_TW + lane;
    s_lab[i] = (uint8_t)c;
    s_par[i] = ly * CC_TW + first;
    s_cnt[i] = 0;
    starts[k] = st;
    mine[k] = c;
  }
  __syncthreads();

  // unite with the row above; a pair of runs is united by its first column only
#pragma unroll
  for (int k = 0; k < CC_ROWS_PER_WAVE; ++k) {
    const int ly = wv + 4 * k;
    const unsigned c = mine[k];
    if (ly == 0 || c >= CC_IGNORED) continue;
    const int i = ly * CC_TW + lane;
    const bool west = lane > 0 && !((starts[k] >> lane) & 1);             // same run as lane - 1
    const bool east = lane < 63 && !((starts[k] >> (lane + 1)) & 1);      // same run as lane + 1
    const bool n = s_lab[i - CC_TW] == c;
    const bool nw = lane > 0 && s_lab[i - CC_TW - 1] == c;
    const bool ne = lane < 63 && s_lab[i - CC_TW + 1] == c;
    if (n && !(west && nw)) cc_lunion(s_par, i, i - CC_TW);               // west && nw: the pair (W, NW) stands for this one
    if (conn8) {
      if (nw && !n && !west) cc_lunion(s_par, i, i - CC_TW - 1);          // n: through N's run; west: the pair (W, NW)
      if (ne && !n && !east) cc_lunion(s_par, i, i - CC_TW + 1);          // east: the pair (E, NE)
    }
  }
  __syncthreads();

  // every run finds its tile-local root once and adds its length and its border bit there
  int root[CC_ROWS_PER_WAVE];
#pragma unroll
  for (int k = 0; k < CC_ROWS_PER_WAVE; ++k) {
    const int ly = wv + 4 * k, gy = y0 + ly;
    const unsigned long long st = starts[k];
    const bool start = (st >> lane) & 1;
    int r = -1;
    if (start && mine[k] < CC_IGNORED) {
      const unsigned long long above = lane == 63 ? 0ull : st & (~0ull << (lane + 1));
      const int end = above ? __builtin_ctzll(above) : 64;                // one past the run's last lane
      r = cc_lfind(s_par, ly * CC_TW + lane);
      const bool edge = gy == 0 || gy == h - 1 || gx == 0 || x0 + end - 1 == w - 1;
      atomicAdd(&s_cnt[r], end - lane);
      if (edge) atomicOr(&s_cnt[r], CC_BORDER);
    }
    const int first = 63 - __builtin_clzll(st & (~0ull >> (63 - lane)));
    root[k] = __shfl(r, first);
  }
  __syncthreads();

#pragma unroll
  for (int k = 0; k < CC_ROWS_PER_WAVE; ++k) {
    const int ly = wv + 4 * k, gy = y0 + ly;
    if (gy >= h || gx >= w) continue;
    const size_t g = base + (size_t)gy * w + gx;
    const int i = ly * CC_TW + lane, r = root[k];
    lab[g] = (uint8_t)mine[k];
    roots[g] = r < 0 ? -1 : (y0 + r / CC_TW) * w + x0 + r % CC_TW;
    info[g] = r == i ? s_cnt[i] : 0;
  }
}

// ---- border ------------------------------------------------------------------------------------------------------------------
// per image (nty - 1) * w pixels of first tile rows, then (ntx - 1) * h pixels of first tile columns
__global__ void __launch_bounds__(256) cc_border_kernel(const uint8_t* __restrict__ lab, int* roots, int h, int w, int conn8, int ntx,
                                                        int nty, size_t per_image, size_t total) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const size_t img = t / per_image;
  const size_t k = t - img * per_image;
  const size_t nrow = (size_t)(nty - 1) * w;
  const uint8_t* L = lab + img * (size_t)h * w;
  int* P = roots + img * (size_t)h * w;
  if (k < nrow) {                                      // first row of a tile: the row above belongs to another tile
    const int y = ((int)(k / (size_t)w) + 1) * CC_TH, x = (int)(k % (size_t)w);
    const int i = y * w + x;
    const unsigned c = L[i];
    if (c >= CC_IGNORED) return;
    // as in the local pass a pair of runs is united once: neighbours along the edge inside one tile are united already
    const bool n = L[i - w] == c;
    const bool nw = x > 0 && L[i - w - 1] == c, ne = x + 1 < w && L[i - w + 1] == c;
    const bool west = x % CC_TW != 0 && L[i - 1] == c;                    // W in this tile and this run; NW then in N's tile
    const bool east = (x + 1) % CC_TW != 0 && x + 1 < w && L[i + 1] == c;
    if (n && !(west && nw)) cc_gunion(P, i, i - w);                       // west && nw: W's thread unites (W, NW)
    if (conn8) {
      if (nw && !n && !west) cc_gunion(P, i, i - w - 1);                  // n: N and NW are united (local or border); west: (W, NW)
      if (ne && !n && !east) cc_gunion(P, i, i - w + 1);                  // east: E's thread unites (E, NE)
    }
  } else {                                             // first column of a tile: the column to the left belongs to another
    const size_t kk = k - nrow;
    const int x = ((int)(kk / (size_t)h) + 1) * CC_TW, y = (int)(kk % (size_t)h);
    const int i = y * w + x;
    const unsigned c = L[i];
    if (c >= CC_IGNORED) return;
    const bool wst = L[i - 1] == c;
    const bool nw = y > 0 && L[i - w - 1] == c, sw = y + 1 < h && L[i + w - 1] == c;
    const bool north = y % CC_TH != 0 && L[i - w] == c;                   // N in this tile: united with this pixel, NW with W
    const bool south = (y + 1) % CC_TH != 0 && y + 1 < h && L[i + w] == c;
    if (wst && !(north && nw)) cc_gunion(P, i, i - 1);                    // north && nw: N's thread unites (N, NW)
    if (conn8) {
      if (nw && !wst && !north) cc_gunion(P, i, i - w - 1);               // wst: W and NW are united (local or border); north: (N, NW)
      if (sw && !wst && !south) cc_gunion(P, i, i + w - 1);               // south: S's thread unites (S, SW)
    }
  }
}

// ---- flatten -----------------------------------------------------------------------------------------------------------------
// Nothing links here: the roots are fixed, a walk through a parent that another thread has already flattened only gets shorter.
__global__ void __launch_bounds__(256) cc_flatten_kernel(int* roots, int* info, size_t hw, size_t total) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const size_t img = t / hw;
  const int i = (int)(t - img * hw);
  int* P = roots + img * hw;
  int* F = info + img * hw;
  const int p = __hip_atomic_load(&P[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (p < 0 || p == i) return;                         // outside, or a root: it keeps its own counter
  const int r = cc_gfind(P, p);
  if (r != p) __hip_atomic_store(&P[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int v = F[i];                                  // non-zero: a tile-local root; only this thread touches F[i]
  if (v) {
    atomicAdd(&F[r], v & CC_AREA_MASK);
    if (v & CC_BORDER) atomicOr(&F[r], CC_BORDER);
    F[i] = 0;
  }
}

// ---- filter ------------------------------------------------------------------------------------------------------------------
struct CcRulesDev {
  int min_area[OCT_MAX_CLASSES];
  long long replace[OCT_MAX_CLASSES];
  unsigned keep_largest, drop_enclosed;                // bit c
};

template <typename T>
__global__ void __launch_bounds__(256) cc_best_kernel(const T* __restrict__ map, const int* __restrict__ info,
                                                      unsigned long long* __restrict__ best, size_t hw, size_t total, int C,
                                                      unsigned keep_largest) {
  // Noise has a root every few pixels and only images * C slots: the keys of a workgroup meet in LDS first, and a key goes to
  // the slot only when it beats what the slot is seen to hold.  The slot only grows, so a stale reading is a lower bound: it
  // can cost an atomic that changes nothing, never drop the maximum.
  __shared__ unsigned long long s_best[OCT_MAX_CLASSES];
  const int tid = threadIdx.x;
  const size_t t0 = (size_t)blockIdx.x * 256, t = t0 + tid;
  const size_t last = t0 + 255 < total ? t0 + 255 : total - 1;
  const size_t img0 = t0 / hw;
  const bool one_image = img0 == last / hw;            // block-uniform
  unsigned long long key = 0ull;
  unsigned c = 0u;
  size_t img = img0;
  if (t < total) {
    const int v = info[t];
    if (v) {                                           // a root: inside, so its class is below C; checked before it indexes
      c = (unsigned)map[t];
      if (c < (unsigned)C && ((keep_largest >> c) & 1)) {
        img = t / hw;
        const unsigned root = (unsigned)(t - img * hw);
        key = ((unsigned long long)(unsigned)(v & CC_AREA_MASK) << 32) | (0xFFFFFFFFu - root);
      }
    }
  }
  if (!one_image) {                                    // images smaller than a workgroup: straight to the slots
    if (key && key > __hip_atomic_load(&best[img * C + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(&best[img * C + c], key);
    return;
  }
  if (tid < OCT_MAX_CLASSES) s_best[tid] = 0ull;
  __syncthreads();
  if (key) atomicMax(&s_best[c], key);
  __syncthreads();
  if (tid < C) {
    const unsigned long long k = s_best[tid];
    if (k && k > __hip_atomic_load(&best[img0 * C + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(&best[img0 * C + tid], k);
  }
}

template <typename T>
__global__ void __launch_bounds__(256) cc_apply_kernel(const T* map, const int* __restrict__ roots, const int* __restrict__ info,
                                                       const unsigned long long* __restrict__ best, T* out, size_t hw, size_t total,
                                                       int C, const CcRulesDev rules) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const T v = map[t];
  const int r = roots[t];
  T res = v;
  if (r >= 0) {
    const unsigned c = (unsigned)v;
    const size_t img = t / hw;
    if (c < (unsigned)C) {                             // always, for roots written by oct_cc_label with this descriptor
      const int f = info[img * hw + r];
      const int area = f & CC_AREA_MASK;
      bool drop = area < rules.min_area[c];
      if ((rules.keep_largest >> c) & 1) drop |= (unsigned)(0xFFFFFFFFu - (unsigned)best[img * C + c]) != (unsigned)r;
      if ((rules.drop_enclosed >> c) & 1) drop |= !(f & CC_BORDER);
      if (drop) res = (T)rules.replace[c];
    }
  }
  out[t] = res;
}

// ---- lesion counts -----------------------------------------------------------------------------------------------------------
// adds 1 at arr[key] for every lane with key >= 0; lanes of a wave that follow each other with one key share the atomic
__device__ __forceinline__ void cc_run_add(int* arr, int key, int lane) {
  const int prev = __shfl_up(key, 1);
  const bool head = lane == 0 || prev != key;
  const unsigned long long heads = __ballot(head);
  if (head && key >= 0) {
    const unsigned long long above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
    const int end = above ? __builtin_ctzll(above) : 64;
    atomicAdd(&arr[key], end - lane);
  }
}

// inter: per component the pixels on which both maps carry its class.  Keys are indices into [images][h][w] (below 2^31).
__global__ void __launch_bounds__(256) cc_inter_kernel(const uint8_t* __restrict__ lab_t, const uint8_t* __restrict__ lab_p,
                                                       const int* __restrict__ roots_t, const int* __restrict__ roots_p,
                                                       int* inter_t, int* inter_p, size_t hw, size_t total) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int kt = -1, kp = -1;
  if (t < total) {
    const unsigned a = lab_t[t], b = lab_p[t];
    if (a == b && a < CC_IGNORED) {
      const size_t img0 = (t / hw) * hw;
      kt = (int)(img0 + roots_t[t]);
      kp = (int)(img0 + roots_p[t]);
    }
  }
  cc_run_add(inter_t, kt, lane);
  cc_run_add(inter_p, kp, lane);
}

__global__ void __launch_bounds__(256) cc_count_kernel(const uint8_t* __restrict__ lab_t, const uint8_t* __restrict__ lab_p,
                                                       const int* __restrict__ info_t, const int* __restrict__ info_p,
                                                       const int* __restrict__ inter_t, const int* __restrict__ inter_p,
                                                       unsigned long long* __restrict__ state, size_t total, int C, int images,
                                                       long long num, long long den) {
  __shared__ unsigned s_n[OCT_MAX_CLASSES * 4 + 2];    // per class: target, predicted, detected, confirmed; ignored, invalid
  const int tid = threadIdx.x;
  if (tid < OCT_MAX_CLASSES * 4 + 2) s_n[tid] = 0u;
  __syncthreads();
  const size_t t = (size_t)blockIdx.x * 256 + tid;
  if (t < total) {
    const unsigned a = lab_t[t], b = lab_p[t];
    if (a == CC_IGNORED) atomicAdd(&s_n[OCT_MAX_CLASSES * 4], 1u);
    else if (a == CC_NOCLASS || b == CC_NOCLASS) atomicAdd(&s_n[OCT_MAX_CLASSES * 4 + 1], 1u);
    const int ft = info_t[t], fp = info_p[t];
    if (ft && a < (unsigned)C) {                       // a root of the target: a < C before it indexes
      const long long area = ft & CC_AREA_MASK, in = inter_t[t];
      atomicAdd(&s_n[a * 4 + 0], 1u);
      if (in >= 1 && in * den >= num * area) atomicAdd(&s_n[a * 4 + 2], 1u);
    }
    if (fp && b < (unsigned)C) {
      const long long area = fp & CC_AREA_MASK, in = inter_p[t];
      atomicAdd(&s_n[b * 4 + 1], 1u);
      if (in >= 1 && in * den >= num * area) atomicAdd(&s_n[b * 4 + 3], 1u);
    }
  }
  __syncthreads();
  if (tid < C * 4) {
    if (s_n[tid]) atomicAdd(&state[tid], (unsigned long long)s_n[tid]);
  } else if (tid >= OCT_MAX_CLASSES * 4 && tid < OCT_MAX_CLASSES * 4 + 2) {
    if (s_n[tid]) atomicAdd(&state[C * 4 + 1 + (tid - OCT_MAX_CLASSES * 4)], (unsigned long long)s_n[tid]);
  }
  if (blockIdx.x == 0 && tid == 255) {
    atomicAdd(&state[C * 4 + 0], (unsigned long long)images);
    atomicAdd(&state[C * 4 + 3], 1ull);
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
extern "C" size_t oct_cc_workspace_bytes(const OctCcDesc* d) {
  if (cc_check_desc(d, "oct_cc_workspace_bytes") != OCT_OK) return 0;
  CcWs ws;
  cc_layout(d, d->op, &ws);
  return ws.total;
}

extern "C" int oct_cc_tile(int* th, int* tw) {
  OCT_CHECK(th && tw, "oct_cc_tile: null output");
  *th = CC_TH;
  *tw = CC_TW;
  return OCT_OK;
}

// the three launches that label one map: roots / info as the header describes them
static int cc_label_map(const OctCcDesc* d, int elem, int ign_elem, const void* map, const void* ign, uint8_t* lab, int* roots, int* info,
                        hipStream_t s, const char* who) {
  const int h = d->h, w = d->w;
  const int ntx = ceil_div(w, CC_TW), nty = ceil_div(h, CC_TH);
  const size_t tiles = (size_t)d->images * ntx * nty;
  const size_t hw = (size_t)h * w, N = hw * d->images;
  const size_t per_image = (size_t)(nty - 1) * w + (size_t)(ntx - 1) * h;
  const size_t nborder = per_image * d->images;
  OCT_CHECK(tiles < 2147483648ull && (nborder + 255) / 256 < 2147483648ull, "%s: the batch needs more than 2^31 workgroups", who);
  const int conn8 = d->connectivity == 8, has_ignore = d->has_ignore ? 1 : 0;
  const long long ignv = (long long)d->ignore_index;
  const dim3 b(256), gt((unsigned)tiles);
#define CC_LOCAL(T, U)                                                                                                          \
  hipLaunchKernelGGL((cc_local_kernel<T, U>), gt, b, 0, s, reinterpret_cast<const T*>(map), reinterpret_cast<const U*>(ign), lab, \
                     roots, info, h, w, d->classes, conn8, has_ignore, ignv, ntx, nty)
  if (elem == 0) { if (ign_elem == 0) CC_LOCAL(uint8_t, uint8_t); else CC_LOCAL(uint8_t, long long); }
  else { if (ign_elem == 0) CC_LOCAL(long long, uint8_t); else CC_LOCAL(long long, long long); }
#undef CC_LOCAL
  if (nborder)
    hipLaunchKernelGGL(cc_border_kernel, dim3((unsigned)((nborder + 255) / 256)), b, 0, s, lab, roots, h, w, conn8, ntx, nty, per_image,
                       nborder);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)((N + 255) / 256)), b, 0, s, roots, info, hw, N);
  return OCT_OK;
}

static int cc_check_ptr(const void* p, int elem, const char* who, const char* what) {
  OCT_CHECK(p, "%s: null %s", who, what);
  OCT_CHECK(elem == 0 || ((uintptr_t)p & 7) == 0, "%s: int64 %s not 8-byte aligned", who, what);
  return OCT_OK;
}

extern "C" int oct_cc_label(const OctCcDesc* d, const void* map, int32_t* roots, int32_t* info, void* workspace, void* stream) {
  int rc = cc_check_desc(d, "oct_cc_label");
  if (rc != OCT_OK) return rc;
  if (d->images == 0) return OCT_OK;
  if ((rc = cc_check_ptr(map, d->map_elem, "oct_cc_label", "map")) != OCT_OK) return rc;
  OCT_CHECK(roots && info, "oct_cc_label: null output");
  OCT_CHECK((((uintptr_t)roots | (uintptr_t)info) & 3) == 0, "oct_cc_label: roots / info not 4-byte aligned");
  OCT_CHECK(workspace && ((uintptr_t)workspace & 15) == 0, "oct_cc_label: the workspace is null or not 16-byte aligned");
  CcWs ws;
  cc_layout(d, OCT_CC_OP_LABEL, &ws);
  uint8_t* lab = reinterpret_cast<uint8_t*>(workspace) + ws.lab[0];
  rc = cc_label_map(d, d->map_elem, d->map_elem, map, map, lab, roots, info, as_stream(stream), "oct_cc_label");
  if (rc != OCT_OK) return rc;
  return oct_check_launch("cc_label");
}

extern "C" int oct_cc_filter(const OctCcDesc* d, const OctCcRules* rules, const void* map, const int32_t* roots, const int32_t* info,
                             void* out, void* workspace, void* stream) {
  int rc = cc_check_desc(d, "oct_cc_filter");
  if (rc != OCT_OK) return rc;
  OCT_CHECK(rules, "oct_cc_filter: null rules");
  CcRulesDev rd = {};
  for (int c = 0; c < d->classes; ++c) {
    OCT_CHECK(rules->min_area[c] >= 0, "oct_cc_filter: min_area[%d] must not be negative (got %d)", c, rules->min_area[c]);
    OCT_CHECK((rules->keep_largest[c] | 1) == 1 && (rules->drop_enclosed[c] | 1) == 1,
              "oct_cc_filter: keep_largest[%d] and drop_enclosed[%d] must be 0 or 1", c, c);
    OCT_CHECK(d->map_elem != 0 || (rules->replace[c] >= 0 && rules->replace[c] <= 255),
              "oct_cc_filter: replace[%d] = %lld does not fit a uint8 map", c, (long long)rules->replace[c]);
    rd.min_area[c] = rules->min_area[c];
    rd.replace[c] = (long long)rules->replace[c];
    rd.keep_largest |= (unsigned)rules->keep_largest[c] << c;
    rd.drop_enclosed |= (unsigned)rules->drop_enclosed[c] << c;
  }
  if (d->images == 0) return OCT_OK;
  if ((rc = cc_check_ptr(map, d->map_elem, "oct_cc_filter", "map")) != OCT_OK) return rc;
  if ((rc = cc_check_ptr(out, d->map_elem, "oct_cc_filter", "out")) != OCT_OK) return rc;
  OCT_CHECK(roots && info, "oct_cc_filter: null roots / info");
  OCT_CHECK((((uintptr_t)roots | (uintptr_t)info) & 3) == 0, "oct_cc_filter: roots / info not 4-byte aligned");
  OCT_CHECK(workspace && ((uintptr_t)workspace & 15) == 0, "oct_cc_filter: the workspace is null or not 16-byte aligned");
  CcWs ws;
  cc_layout(d, OCT_CC_OP_FILTER, &ws);
  unsigned long long* best = reinterpret_cast<unsigned long long*>(reinterpret_cast<unsigned char*>(workspace) + ws.best);
  hipStream_t s = as_stream(stream);
  const size_t hw = (size_t)d->h * d->w, N = hw * d->images;
  const dim3 b(256), g((unsigned)((N + 255) / 256));
  if (rd.keep_largest) {
    const hipError_t e = hipMemsetAsync(best, 0, 8 * (size_t)d->images * d->classes, s);
    if (e != hipSuccess) {
      oct_set_error("oct_cc_filter: clearing the largest-component slots failed: %s", hipGetErrorString(e));
      return OCT_E_LAUNCH;
    }
    if (d->map_elem == 0)
      hipLaunchKernelGGL(cc_best_kernel<uint8_t>, g, b, 0, s, reinterpret_cast<const uint8_t*>(map), info, best, hw, N, d->classes,
                         rd.keep_largest);
    else
      hipLaunchKernelGGL(cc_best_kernel<long long>, g, b, 0, s, reinterpret_cast<const long long*>(map), info, best, hw, N, d->classes,
                         rd.keep_largest);
  }
  if (d->map_elem == 0)
    hipLaunchKernelGGL(cc_apply_kernel<uint8_t>, g, b, 0, s, reinterpret_cast<const uint8_t*>(map), roots, info, best,
                       reinterpret_cast<uint8_t*>(out), hw, N, d->classes, rd);
  else
    hipLaunchKernelGGL(cc_apply_kernel<long long>, g, b, 0, s, reinterpret_cast<const long long*>(map), roots, info, best,
                       reinterpret_cast<long long*>(out), hw, N, d->classes, rd);
  return oct_check_launch("cc_filter");
}

extern "C" int oct_lesion_eval_update(const OctCcDesc* d, const void* target, const void* pred, int64_t* state, void* workspace,
                                      void* stream) {
  int rc = cc_check_desc(d, "oct_lesion_eval_update");
  if (rc != OCT_OK) return rc;
  if (d->images == 0) return OCT_OK;
  if ((rc = cc_check_ptr(target, d->map_elem, "oct_lesion_eval_update", "target")) != OCT_OK) return rc;
  if ((rc = cc_check_ptr(pred, d->pred_elem, "oct_lesion_eval_update", "prediction")) != OCT_OK) return rc;
  OCT_CHECK(state && ((uintptr_t)state & 7) == 0, "oct_lesion_eval_update: the state is null or not 8-byte aligned");
  OCT_CHECK(workspace && ((uintptr_t)workspace & 15) == 0, "oct_lesion_eval_update: the workspace is null or not 16-byte aligned");
  CcWs ws;
  cc_layout(d, OCT_CC_OP_LESION, &ws);
  unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
  uint8_t* lab[2]; int* roots[2]; int* info[2]; int* inter[2];
  for (int m = 0; m < 2; ++m) {
    lab[m] = base + ws.lab[m];
    roots[m] = reinterpret_cast<int*>(base + ws.roots[m]);
    info[m] = reinterpret_cast<int*>(base + ws.info[m]);
    inter[m] = reinterpret_cast<int*>(base + ws.inter[m]);
  }
  hipStream_t s = as_stream(stream);
  const size_t hw = (size_t)d->h * d->w, N = hw * d->images;
  for (int m = 0; m < 2; ++m) {
    const hipError_t e = hipMemsetAsync(inter[m], 0, 4 * N, s);
    if (e != hipSuccess) {
      oct_set_error("oct_lesion_eval_update: clearing the overlap counters failed: %s", hipGetErrorString(e));
      return OCT_E_LAUNCH;
    }
  }
  // the target's ignore_index puts a pixel outside in both maps
  if ((rc = cc_label_map(d, d->map_elem, d->map_elem, target, target, lab[0], roots[0], info[0], s, "oct_lesion_eval_update")) != OCT_OK)
    return rc;
  if ((rc = cc_label_map(d, d->pred_elem, d->map_elem, pred, target, lab[1], roots[1], info[1], s, "oct_lesion_eval_update")) != OCT_OK)
    return rc;
  const dim3 b(256), g((unsigned)((N + 255) / 256));
  hipLaunchKernelGGL(cc_inter_kernel, g, b, 0, s, lab[0], lab[1], roots[0], roots[1], inter[0], inter[1], hw, N);
  hipLaunchKernelGGL(cc_count_kernel, g, b, 0, s, lab[0], lab[1], info[0], info[1], inter[0], inter[1],
                     reinterpret_cast<unsigned long long*>(state), N, d->classes, d->images, (long long)d->overlap_num,
                     (long long)d->overlap_den);
  return oct_check_launch("lesion_eval_update");
}
