// Contour metrics (oct_contour_update): per image, class and direction the five exact integers behind Hausdorff, HD95 and
// ASSD of a (target, prediction) pair of class maps -- n, max D2, the two order statistics of D2 around the 95th percentile
// and sum floor(2^16 sqrt(D2)) -- written to records[images][C][2][5].
//
// Contour points live on the doubled site grid Hd x Wd = (2h-1) x (2w-1): site (Y, X) with Y + X odd is the midpoint of the
// pixel pair (Y/2, (X-1)/2) | (Y/2, (X+1)/2) (Y even) or ((Y-1)/2, X/2) | ((Y+1)/2, X/2) (Y odd); it is a point of class c when
// exactly one pixel of the pair has label c and neither is ignored.  Since Wd is odd, these sites are the odd linear indices
// i = Y*Wd + X, and k = i >> 1 numbers them densely.  D2 = squared distance in doubled coordinates (true distance sqrt(D2)/2).
//
// One update is a fixed sequence of launches on the caller's stream, every buffer in the caller's workspace:
//   labels   both maps as uint8: class, CT_NOCLASS (outside [0, C)) or CT_IGNORED (target == ignore_index, in BOTH maps)
//   mask     one thread per (map, image, class, column X, segment of 64 site rows): the points of the class as a 64-bit mask;
//            counts the points per (map, image, class)
//   dist     the same threads: g[Y] = vertical distance to the nearest point of that class in the column (CT_FAR: none), by
//            bit scans of the segment's mask and of the nearest non-empty masks above and below; stores only
//   walk     one thread per site: a source point walks outward along its row of the other map's g, r = 0, 1, ... while
//            r^2 < best (at most Wd steps), best = min(r^2 + g^2): the exact D2.  max and sum_q go through LDS to one 64-bit
//            integer atomic per (block, class, direction); D2 is kept per site for the selection
//   select   radix select of the ranks lo = 19(n-1)/20 and hi = min(lo+1, n-1), most significant byte first: four
//            (histogram, scan) rounds over the stored D2, LDS histograms, integer atomics; a round whose byte no D2 of the
//            image reaches (by max_d2) ends at once
// Everything accumulated is an integer: two runs give identical bits.  A label is range-checked before it indexes anything.
#include "common.h"

#define CT_NOCLASS 0xFFu
#define CT_IGNORED 0xFEu
#define CT_FAR 0xFFFFu          // g: no point of the class in this column
#define CT_NONE 0xFFFFFFFFu     // D2 slot: not a source point (or the other side has no point)
#define CT_MAX_DIM 16384        // D2 <= 2 * 32766^2 < 2^31
#define CT_WALK_PER 4           // sites per thread, walk
#define CT_HIST_PER 16          // sites per thread, histogram rounds

struct ContourGeom {
  int images, h, w, C, hd, wd;
  size_t nhalf;   // candidate sites per image: odd linear indices of the hd x wd grid
};

struct ContourWs {   // byte offsets into the workspace
  size_t lab, g, mask, d2, npts, sel, hist, total;
};

static inline size_t ct_align(size_t v) { return (v + 255) & ~(size_t)255; }
static inline size_t ct_segments(int hd) { return ((size_t)hd + 63) / 64; }   // 64 site rows per mask

static void ct_layout(const OctContourDesc* d, ContourGeom* ge, ContourWs* ws) {
  ge->images = d->images; ge->h = d->h; ge->w = d->w; ge->C = d->classes;
  ge->hd = 2 * d->h - 1; ge->wd = 2 * d->w - 1;
  ge->nhalf = ((size_t)ge->hd * ge->wd) >> 1;
  const size_t I = (size_t)d->images, C = (size_t)d->classes, R = I * C * 2;
  size_t o = 0;
  ws->lab = o;  o += ct_align(2 * I * d->h * d->w);                          // uint8 [2][I][h][w]
  ws->g = o;    o += ct_align(2 * I * C * ge->hd * ge->wd * sizeof(uint16_t));   // [2][I][C][hd][wd]
  ws->mask = o; o += ct_align(2 * I * C * ct_segments(ge->hd) * ge->wd * sizeof(unsigned long long));   // [2][I][C][nseg][wd]
  ws->d2 = o;   o += ct_align(2 * I * ge->nhalf * 2 * sizeof(unsigned));     // [2 dir][I][nhalf][2 slots]
  ws->npts = o; o += ct_align(2 * I * C * sizeof(unsigned));                 // [2 map][I][C]
  ws->sel = o;  o += ct_align(R * 2 * 2 * sizeof(unsigned));                 // [R][2 ranks]{prefix, rank}
  ws->hist = o; o += ct_align(R * 2 * 256 * sizeof(unsigned));               // [R][2 ranks][256]
  ws->total = o;
}

static int ct_check_desc(const OctContourDesc* d, const char* who) {
  OCT_CHECK(d, "%s: null descriptor", who);
  OCT_CHECK(d->classes >= 1 && d->classes <= OCT_MAX_CLASSES, "%s: classes must be 1..%d (got %d)", who, OCT_MAX_CLASSES, d->classes);
  OCT_CHECK(d->images >= 0 && d->h >= 1 && d->w >= 1, "%s: bad geometry %d x %d x %d", who, d->images, d->h, d->w);
  OCT_CHECK(d->h <= CT_MAX_DIM && d->w <= CT_MAX_DIM, "%s: h and w must not exceed %d (got %d x %d)", who, CT_MAX_DIM, d->h, d->w);
  OCT_CHECK((double)d->images * d->h * d->w < 2147483648.0, "%s: images * h * w must stay below 2^31", who);
  OCT_CHECK(d->target_elem == 0 || d->target_elem == 2, "%s: target class maps are uint8 (0) or int64 (2), got %d", who, d->target_elem);
  OCT_CHECK(d->pred_elem == 0 || d->pred_elem == 2, "%s: predicted class maps are uint8 (0) or int64 (2), got %d", who, d->pred_elem);
  return OCT_OK;
}

// ---- labels --------------------------------------------------------------------------------------------------------------
template <typename TT, typename PT>
__global__ void __launch_bounds__(256) contour_labels_kernel(const TT* __restrict__ target, const PT* __restrict__ pred,
                                                             uint8_t* __restrict__ lab, size_t npix, int C, int has_ignore,
                                                             long long ignore_index) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const long long t = (long long)target[i], p = (long long)pred[i];
  const bool ign = has_ignore && t == ignore_index;
  lab[i] = ign ? CT_IGNORED : (unsigned long long)t < (unsigned long long)C ? (uint8_t)t : CT_NOCLASS;
  lab[npix + i] = ign ? CT_IGNORED : (unsigned long long)p < (unsigned long long)C ? (uint8_t)p : CT_NOCLASS;
}

// the two labels of site (Y, X), Y + X odd, of one image's uint8 map: always two in-image pixels
__device__ __forceinline__ void ct_site_labels(const uint8_t* img_lab, int w, int Y, int X, unsigned* la, unsigned* lb) {
  const size_t a = (size_t)(Y >> 1) * w + (X >> 1);
  *la = img_lab[a];
  *lb = img_lab[a + ((Y & 1) ? w : 1)];
}

// ---- column distances ------------------------------------------------------------------------------------------------------
// A column of the site grid in segments of 64 site rows: the points of one class in a segment are one 64-bit mask.
// blockIdx.x = (col * nseg + seg) * strips + strip with col = (map * images + img) * C + c; a thread owns one X of the strip.
__global__ void __launch_bounds__(256) contour_mask_kernel(const uint8_t* __restrict__ lab, unsigned long long* __restrict__ mask,
                                                           unsigned* __restrict__ npts, const ContourGeom ge, int strips, int nseg) {
  const int strip = (int)(blockIdx.x % (unsigned)strips);
  const size_t cs = blockIdx.x / (unsigned)strips;    // col * nseg + seg
  const int seg = (int)(cs % (size_t)nseg);
  const size_t col = cs / (size_t)nseg;
  const unsigned c = (unsigned)(col % (size_t)ge.C);
  const size_t mi = col / (size_t)ge.C;               // map * images + img
  const int X = strip * 256 + (int)threadIdx.x;
  unsigned count = 0;
  if (X < ge.wd) {
    const int h = ge.h, w = ge.w;
    const bool odd = X & 1;                            // odd X: points at even Y (pixel pair along the row), even X: at odd Y
    const uint8_t* la = lab + mi * (size_t)h * w + (X >> 1);
    const size_t step = odd ? 1 : (size_t)w;
    unsigned long long m = 0ull;
#pragma unroll 8
    for (int j = 0; j < 32; ++j) {                     // pixel row y holds site rows 2y and 2y + 1 of the segment
      const int y = 32 * seg + j;
      const bool pair = y < h && (odd || y + 1 < h);
      const int yc = y < h ? y : h - 1;                // clamped: every load is in bounds
      const unsigned a = la[(size_t)yc * w], b = pair ? la[(size_t)yc * w + step] : a;
      const bool pt = pair && a != CT_IGNORED && b != CT_IGNORED && ((a == c) != (b == c));
      if (pt) m |= 1ull << (2 * j + (odd ? 0 : 1));
    }
    mask[cs * (size_t)ge.wd + X] = m;
    count = (unsigned)__popcll(m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o);
  if ((threadIdx.x & 63) == 0 && count) atomicAdd(&npts[col], count);
}

// g[Y] = vertical distance to the nearest point of the class in the column (CT_FAR: none): inside the segment by bit scans
// of its mask, beyond it from the nearest non-empty segment above and below (at most nseg steps each way)
__global__ void __launch_bounds__(256) contour_dist_kernel(const unsigned long long* __restrict__ mask, uint16_t* __restrict__ g,
                                                           const ContourGeom ge, int strips, int nseg) {
  const int strip = (int)(blockIdx.x % (unsigned)strips);
  const size_t cs = blockIdx.x / (unsigned)strips;
  const int seg = (int)(cs % (size_t)nseg);
  const size_t col = cs / (size_t)nseg;
  const int X = strip * 256 + (int)threadIdx.x;
  if (X >= ge.wd) return;
  const int wd = ge.wd, hd = ge.hd;
  const unsigned long long* mc = mask + col * (size_t)nseg * wd + X;
  const unsigned long long m = mc[(size_t)seg * wd];
  int above = -1, below = -1;                          // site rows of the nearest points outside the segment
  for (int s = seg - 1; s >= 0; --s) {
    const unsigned long long v = mc[(size_t)s * wd];
    if (v) { above = 64 * s + 63 - __builtin_clzll(v); break; }
  }
  for (int s = seg + 1; s < nseg; ++s) {
    const unsigned long long v = mc[(size_t)s * wd];
    if (v) { below = 64 * s + __builtin_ctzll(v); break; }
  }
  uint16_t* gc = g + col * (size_t)hd * wd + X;
  const int y0 = 64 * seg;
#pragma unroll 8
  for (int j = 0; j < 64; ++j) {
    const int Y = y0 + j;
    if (Y >= hd) break;
    const unsigned long long le = m & (~0ull >> (63 - j)), ge_ = m >> j;
    unsigned up = CT_FAR, dn = CT_FAR;
    if (le) up = (unsigned)(j - (63 - __builtin_clzll(le)));
    else if (above >= 0) up = (unsigned)(Y - above);
    if (ge_) dn = (unsigned)__builtin_ctzll(ge_);
    else if (below >= 0) dn = (unsigned)(below - Y);
    gc[(size_t)Y * wd] = (uint16_t)(up < dn ? up : dn);
  }
}

// ---- ranks ---------------------------------------------------------------------------------------------------------------
// record r = (img * C + c) * 2 + dir; dir 0: the points of pred (map 1) against target (map 0), dir 1 the reverse
__global__ void __launch_bounds__(256) contour_ranks_kernel(const unsigned* __restrict__ npts, unsigned* __restrict__ sel,
                                                            unsigned long long* __restrict__ records, int images, int C) {
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= (size_t)images * C * 2) return;
  const int dir = (int)(r & 1);
  const size_t ic = r >> 1;                            // img * C + c
  const size_t src = dir == 0 ? (size_t)images * C : 0, oth = dir == 0 ? 0 : (size_t)images * C;
  const unsigned n = npts[src + ic], m = npts[oth + ic];
  records[r * 5] = n;
  unsigned lo = CT_NONE, hi = CT_NONE;                 // CT_NONE: nothing to select
  if (n && m) {
    lo = (unsigned)((19ull * (n - 1)) / 20ull);
    hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
  }
  sel[r * 4 + 0] = 0u; sel[r * 4 + 1] = lo;
  sel[r * 4 + 2] = 0u; sel[r * 4 + 3] = hi;
}

// ---- walk ----------------------------------------------------------------------------------------------------------------
// floor(2^16 sqrt(d2)) = isqrt(d2 << 32), exact: the double square root is within one of it, two bounded corrections
__device__ __forceinline__ unsigned long long ct_sqrt_q16(unsigned d2) {
  const unsigned long long v = (unsigned long long)d2 << 32;   // at most 31 significant bits: exact as a double
  unsigned long long q = (unsigned long long)sqrt((double)v);
#pragma unroll
  for (int k = 0; k < 2; ++k) if (q * q > v) --q;
#pragma unroll
  for (int k = 0; k < 2; ++k) if ((q + 1) * (q + 1) <= v) ++q;
  return q;
}

__global__ void __launch_bounds__(256) contour_walk_kernel(const uint8_t* __restrict__ lab, const uint16_t* __restrict__ g,
                                                           const unsigned* __restrict__ npts, unsigned* __restrict__ d2,
                                                           unsigned long long* __restrict__ records, const ContourGeom ge,
                                                           int blocks_per_image) {
  __shared__ unsigned s_max[2][OCT_MAX_CLASSES];
  __shared__ unsigned long long s_sum[2][OCT_MAX_CLASSES];
  __shared__ unsigned s_other[2][OCT_MAX_CLASSES];     // points of the other side per (dir, class)
  const int tid = threadIdx.x;
  const int img = (int)(blockIdx.x / (unsigned)blocks_per_image), blk = (int)(blockIdx.x % (unsigned)blocks_per_image);
  const int C = ge.C, wd = ge.wd;
  if (tid < 2 * OCT_MAX_CLASSES) {
    const int dir = tid / OCT_MAX_CLASSES, c = tid % OCT_MAX_CLASSES;
    s_max[dir][c] = 0u; s_sum[dir][c] = 0ull;
    s_other[dir][c] = c < C ? npts[((size_t)(dir == 0 ? 0 : 1) * ge.images + img) * C + c] : 0u;
  }
  __syncthreads();
  const size_t npix = (size_t)ge.h * ge.w, sites = (size_t)ge.hd * wd;
  for (int j = 0; j < CT_WALK_PER; ++j) {
    const size_t k = ((size_t)blk * CT_WALK_PER + j) * 256 + tid;
    if (k >= ge.nhalf) break;
    const size_t i = 2 * k + 1;
    const int Y = (int)(i / (size_t)wd), X = (int)(i - (size_t)Y * wd);
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
      const int smap = dir == 0 ? 1 : 0, omap = 1 - smap;
      unsigned l[2];
      ct_site_labels(lab + ((size_t)smap * ge.images + img) * npix, ge.w, Y, X, &l[0], &l[1]);
      const bool pt = l[0] != l[1] && l[0] != CT_IGNORED && l[1] != CT_IGNORED;
      unsigned out[2] = {CT_NONE, CT_NONE};
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const unsigned c = l[s];
        if (!pt || c >= (unsigned)C || s_other[dir][c] == 0u) continue;   // c < C <= 16 before it indexes
        const uint16_t* row = g + ((((size_t)omap * ge.images + img) * C + c) * sites + (size_t)Y * wd);
        unsigned best = CT_NONE;
        for (int r = 0; r < wd; ++r) {                 // at most the row length
          const unsigned rr = (unsigned)r * (unsigned)r;
          if (rr >= best) break;
          if (X - r >= 0) {
            const unsigned gv = row[X - r];
            if (gv != CT_FAR) { const unsigned v = rr + gv * gv; best = v < best ? v : best; }
          }
          if (r > 0 && X + r < wd) {
            const unsigned gv = row[X + r];
            if (gv != CT_FAR) { const unsigned v = rr + gv * gv; best = v < best ? v : best; }
          }
        }
        out[s] = best;                                 // found: s_other > 0 and the row covers every column
        atomicMax(&s_max[dir][c], best);
        atomicAdd(&s_sum[dir][c], ct_sqrt_q16(best));
      }
      uint2 st; st.x = out[0]; st.y = out[1];
      reinterpret_cast<uint2*>(d2)[((size_t)dir * ge.images + img) * ge.nhalf + k] = st;
    }
  }
  __syncthreads();
  if (tid < 2 * OCT_MAX_CLASSES) {
    const int dir = tid / OCT_MAX_CLASSES, c = tid % OCT_MAX_CLASSES;
    if (c < C) {
      unsigned long long* rec = records + (((size_t)img * C + c) * 2 + dir) * 5;
      if (s_max[dir][c]) atomicMax(&rec[1], (unsigned long long)s_max[dir][c]);
      if (s_sum[dir][c]) atomicAdd(&rec[4], s_sum[dir][c]);
    }
  }
}

// ---- select --------------------------------------------------------------------------------------------------------------
// one round: the byte at `shift` of every D2 whose higher bytes equal the record's prefix, counted per (record, rank)
__global__ void __launch_bounds__(256) contour_hist_kernel(const uint8_t* __restrict__ lab, const unsigned* __restrict__ d2,
                                                           const unsigned* __restrict__ sel, unsigned* __restrict__ hist,
                                                           const unsigned long long* __restrict__ records,
                                                           const ContourGeom ge, int blocks_per_image, int shift) {
  __shared__ unsigned s_hist[OCT_MAX_CLASSES * 2 * 256];
  __shared__ unsigned s_prefix[OCT_MAX_CLASSES][2];
  __shared__ int s_any;
  const int tid = threadIdx.x, dir = blockIdx.y;
  const int img = (int)(blockIdx.x / (unsigned)blocks_per_image), blk = (int)(blockIdx.x % (unsigned)blocks_per_image);
  const int C = ge.C, wd = ge.wd;
  // no D2 of this image and direction reaches this byte (max_d2 is final since the walk): every digit is 0, the empty bins
  // leave prefix and rank as they are, which is the answer of this round
  if (tid == 0) s_any = 0;
  __syncthreads();
  if (tid < C && (records[(((size_t)img * C + tid) * 2 + dir) * 5 + 1] >> shift) != 0ull) atomicOr(&s_any, 1);
  __syncthreads();
  if (!s_any) return;                                  // block-uniform
  for (int i = tid; i < C * 512; i += 256) s_hist[i] = 0u;
  if (tid < 2 * C) {
    const int c = tid >> 1, j = tid & 1;
    s_prefix[c][j] = sel[((((size_t)img * C + c) * 2 + dir) * 2 + j) * 2];
  }
  __syncthreads();
  const size_t npix = (size_t)ge.h * ge.w;
  const uint8_t* slab = lab + ((size_t)(dir == 0 ? 1 : 0) * ge.images + img) * npix;
  const uint2* src = reinterpret_cast<const uint2*>(d2) + ((size_t)dir * ge.images + img) * ge.nhalf;
  for (int jj = 0; jj < CT_HIST_PER; ++jj) {
    const size_t k = ((size_t)blk * CT_HIST_PER + jj) * 256 + tid;
    if (k >= ge.nhalf) break;
    const uint2 v = src[k];
    if (v.x == CT_NONE && v.y == CT_NONE) continue;
    const size_t i = 2 * k + 1;
    const int Y = (int)(i / (size_t)wd), X = (int)(i - (size_t)Y * wd);
    unsigned l[2];
    ct_site_labels(slab, ge.w, Y, X, &l[0], &l[1]);
    const unsigned val[2] = {v.x, v.y};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (val[s] == CT_NONE || l[s] >= (unsigned)C) continue;
      const unsigned high = (unsigned)((unsigned long long)val[s] >> (shift + 8)), digit = (val[s] >> shift) & 255u;
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if (high == (unsigned)((unsigned long long)s_prefix[l[s]][j] >> (shift + 8)))
          atomicAdd(&s_hist[(l[s] * 2 + j) * 256 + digit], 1u);
    }
  }
  __syncthreads();
  for (int i = tid; i < C * 512; i += 256) {
    const unsigned n = s_hist[i];
    if (n) {
      const int c = i >> 9, j = (i >> 8) & 1, digit = i & 255;
      atomicAdd(&hist[((((size_t)img * C + c) * 2 + dir) * 2 + j) * 256 + digit], n);
    }
  }
}

// one wave per (record, rank): the byte whose bin holds the rank; the bins are zeroed for the next round
__global__ void __launch_bounds__(64) contour_scan_kernel(unsigned* __restrict__ sel, unsigned* __restrict__ hist,
                                                          unsigned long long* __restrict__ records, int shift) {
  const size_t rj = blockIdx.x;                        // record * 2 + rank
  const int lane = threadIdx.x;
  unsigned* bins = hist + rj * 256 + 4 * lane;
  const uint4 q = *reinterpret_cast<const uint4*>(bins);
  *reinterpret_cast<uint4*>(bins) = make_uint4(0u, 0u, 0u, 0u);
  const unsigned rank = sel[rj * 2 + 1];
  if (rank == CT_NONE) return;                         // wave-uniform
  const unsigned cnt[4] = {q.x, q.y, q.z, q.w};
  const unsigned own = q.x + q.y + q.z + q.w;
  unsigned incl = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  const unsigned excl = incl - own;
  if (rank >= excl && rank < incl) {                   // exactly one lane: the bins count every value with this prefix
    unsigned rem = rank - excl, digit = 4 * lane + 3;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (rem < cnt[t]) { digit = 4 * lane + t; break; }
      rem -= cnt[t];
    }
    const unsigned prefix = sel[rj * 2] | (digit << shift);
    sel[rj * 2] = prefix;
    sel[rj * 2 + 1] = rem;
    if (shift == 0) records[(rj >> 1) * 5 + 2 + (rj & 1)] = prefix;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
extern "C" size_t oct_contour_workspace_bytes(const OctContourDesc* d) {
  if (ct_check_desc(d, "oct_contour_workspace_bytes") != OCT_OK) return 0;
  ContourGeom ge; ContourWs ws;
  ct_layout(d, &ge, &ws);
  return ws.total;
}

#define CT_HIP(call, what)                                                              \
  do {                                                                                  \
    const hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess) {                                                             \
      oct_set_error("oct_contour_update: %s failed: %s", what, hipGetErrorString(e_));  \
      return OCT_E_LAUNCH;                                                              \
    }                                                                                   \
  } while (0)

extern "C" int oct_contour_update(const OctContourDesc* d, const void* target, const void* pred, int64_t* records, void* workspace,
                                  void* stream) {
  const int rc = ct_check_desc(d, "oct_contour_update");
  if (rc != OCT_OK) return rc;
  if (d->images == 0) return OCT_OK;
  OCT_CHECK(target && pred, "oct_contour_update: null input");
  OCT_CHECK(records, "oct_contour_update: null records");
  OCT_CHECK(workspace, "oct_contour_update: null workspace");
  OCT_CHECK(((uintptr_t)workspace & 15) == 0, "oct_contour_update: workspace not 16-byte aligned");
  OCT_CHECK(((uintptr_t)records & 7) == 0, "oct_contour_update: records not 8-byte aligned");
  OCT_CHECK(d->target_elem == 0 || ((uintptr_t)target & 7) == 0, "oct_contour_update: int64 target not 8-byte aligned");
  OCT_CHECK(d->pred_elem == 0 || ((uintptr_t)pred & 7) == 0, "oct_contour_update: int64 prediction not 8-byte aligned");
  ContourGeom ge; ContourWs ws;
  ct_layout(d, &ge, &ws);
  const size_t I = (size_t)d->images, C = (size_t)d->classes, R = I * C * 2;
  const int strips = ceil_div(ge.wd, 256);
  const int nseg = (int)ct_segments(ge.hd);
  const size_t sweep_blocks = 2 * I * C * nseg * strips;
  const size_t walk_bpi = (ge.nhalf + 256 * CT_WALK_PER - 1) / (256 * CT_WALK_PER);
  const size_t hist_bpi = (ge.nhalf + 256 * CT_HIST_PER - 1) / (256 * CT_HIST_PER);
  OCT_CHECK(sweep_blocks < 2147483648ull && I * walk_bpi < 2147483648ull && R * 2 < 2147483648ull,
            "oct_contour_update: the batch needs more than 2^31 workgroups: pass fewer images per call");
  hipStream_t s = as_stream(stream);
  unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
  uint8_t* lab = base + ws.lab;
  uint16_t* g = reinterpret_cast<uint16_t*>(base + ws.g);
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(base + ws.mask);
  unsigned* d2 = reinterpret_cast<unsigned*>(base + ws.d2);
  unsigned* npts = reinterpret_cast<unsigned*>(base + ws.npts);
  unsigned* sel = reinterpret_cast<unsigned*>(base + ws.sel);
  unsigned* hist = reinterpret_cast<unsigned*>(base + ws.hist);
  unsigned long long* rec = reinterpret_cast<unsigned long long*>(records);

  CT_HIP(hipMemsetAsync(records, 0, R * 5 * sizeof(int64_t), s), "clearing the records");
  CT_HIP(hipMemsetAsync(npts, 0, ws.total - ws.npts, s), "clearing the counters");   // npts | sel | hist are contiguous
  const size_t npix = I * d->h * d->w;
  const dim3 b(256), gl((unsigned)((npix + 255) / 256));
  const int has_ignore = d->has_ignore ? 1 : 0;
  const long long ign = (long long)d->ignore_index;
#define CT_LABELS(TT, PT)                                                                                                        \
  hipLaunchKernelGGL((contour_labels_kernel<TT, PT>), gl, b, 0, s, reinterpret_cast<const TT*>(target),                        \
                     reinterpret_cast<const PT*>(pred), lab, npix, d->classes, has_ignore, ign)
  if (d->target_elem == 0) { if (d->pred_elem == 0) CT_LABELS(uint8_t, uint8_t); else CT_LABELS(uint8_t, long long); }
  else { if (d->pred_elem == 0) CT_LABELS(long long, uint8_t); else CT_LABELS(long long, long long); }
#undef CT_LABELS
  hipLaunchKernelGGL(contour_mask_kernel, dim3((unsigned)sweep_blocks), b, 0, s, lab, mask, npts, ge, strips, nseg);
  hipLaunchKernelGGL(contour_dist_kernel, dim3((unsigned)sweep_blocks), b, 0, s, mask, g, ge, strips, nseg);
  hipLaunchKernelGGL(contour_ranks_kernel, dim3((unsigned)((R + 255) / 256)), b, 0, s, npts, sel, rec, d->images, d->classes);
  if (ge.nhalf > 0) {
    hipLaunchKernelGGL(contour_walk_kernel, dim3((unsigned)(I * walk_bpi)), b, 0, s, lab, g, npts, d2, rec, ge, (int)walk_bpi);
    for (int shift = 24; shift >= 0; shift -= 8) {
      hipLaunchKernelGGL(contour_hist_kernel, dim3((unsigned)(I * hist_bpi), 2), b, 0, s, lab, d2, sel, hist, rec, ge, (int)hist_bpi,
                         shift);
      hipLaunchKernelGGL(contour_scan_kernel, dim3((unsigned)(R * 2)), dim3(64), 0, s, sel, hist, rec, shift);
    }
  }
  return oct_check_launch("contour_update");
}
