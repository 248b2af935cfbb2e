// Distance maps (oct_dt_squared, oct_dt_weight_map, oct_dt_signed): the exact squared Euclidean distance of every pixel of a
// class map to the nearest site of a plane, and the two maps a training step makes of it.  Contract: include/oct_hip.h;
// schedule and bytes: DESIGN.md.
//
// A pixel is valid when its value is in [0, C) and is not ignore_index.  A plane names its sites: the boundary pixels (valid,
// with an in-image 4-neighbour that is valid and differs), the pixels of a class, or the valid pixels of every other class.
// The transform is separable on the plain pixel grid, a fixed sequence of launches on the caller's stream:
//   labels   int64 maps only: the map as bytes (the class, or DT_NONE for an invalid pixel), once for all planes.  A uint8 map
//            is read as it lies, through the same validity rule
//   mask     one thread per (plane, image, column x, segment of DT_SEG rows): the sites of the column as a 64-bit mask; adjacent
//            lanes own adjacent columns, every row read is coalesced.  A wave that saw a site sets the (plane, image) flag
//   dist     the same threads: g[y] = vertical distance to the nearest site of the column (DT_GFAR: none) by bit scans of the
//            segment's mask and of the nearest non-empty masks above and below; stores only
//   rows     one workgroup per DT_ROW_PIX pixels of an (image, plane): whole rows where rows are shorter than that, a stretch
//            of one row otherwise.  The g rows it covers lie in LDS (a long row whole, in each of its workgroups) in blocks of
//            DT_BLK columns with each block's smallest g.  A pixel takes best = min of (x - c)^2 + g[c]^2 over the few columns
//            next to it, then over its own block, then goes outward block by block while a block's nearest column is closer
//            than sqrt(best), and reads a block only where that distance squared plus the block's smallest g squared is below
//            best: every column that could lower the minimum is read, so the result is exact; flat stretches of g are skipped.
//            The epilogue stores int32 D2, fp32 table[min(D2, len - 1)], or the signed fp32 distance (two g planes per class,
//            one search per pixel).  A (plane, image) without a site is answered from its flag
// Integers throughout; the one atomic is the flag's atomicOr.  Two runs give identical bits.
#include "common.h"

#define DT_SEG 64                // rows per column-pass unit: one 64-bit mask
#define DT_ROW_PIX 1024          // pixels per row-pass workgroup: whole rows, or a stretch of a longer row
#define DT_NONE 0xFFu            // label byte of an invalid pixel
#define DT_GFAR 0xFFFFu          // g: no site in this column
#define DT_LNONE 0x8000u         // the same in LDS: DT_LNONE^2 == OCT_DT_FAR
#define DT_BLK 16                // columns per block of a staged row: 32 bytes, two 16-byte LDS reads
#define DT_NEAR 3                // columns each way a pixel looks at one by one before it goes by blocks
#define DT_MAX_DIM 16384         // g fits uint16, a g row fits 32 KiB of LDS, D2 <= 2 * 16383^2 < 2^30
#define DT_SIGNED_MAX (OCT_DT_MAX_PLANES / 2)
#define DT_EPI_SQUARED 0
#define DT_EPI_TABLE 1
#define DT_EPI_SIGNED 2

static_assert(DT_ROW_PIX % 256 == 0 && DT_MAX_DIM * 2 <= 32 * 1024, "a 256-thread workgroup, a g row within 32 KiB of LDS");
static_assert(DT_LNONE * DT_LNONE == OCT_DT_FAR && DT_MAX_DIM <= DT_LNONE && DT_MAX_DIM % DT_BLK == 0 && DT_ROW_PIX % DT_BLK == 0,
              "no-site columns square to OCT_DT_FAR, above every real g; whole blocks at the largest sizes");
static_assert(2 * (DT_MAX_DIM - 1) * (DT_MAX_DIM - 1) < OCT_DT_FAR, "every real D2 lies below OCT_DT_FAR");

struct DtPlanes {    // the site set of every g plane, by value to the kernels
  uint8_t kind[OCT_DT_MAX_PLANES], cls[OCT_DT_MAX_PLANES];
};

struct DtWs {        // byte offsets into the workspace
  size_t lab, g, mask, flags, total;
};

static inline size_t dt_align(size_t v) { return (v + 255) & ~(size_t)255; }
static inline int dt_gplanes(const OctDtDesc* d, int op) { return op == OCT_DT_OP_SIGNED ? 2 * d->planes : d->planes; }

static void dt_layout(const OctDtDesc* d, int op, DtWs* ws) {
  const size_t I = (size_t)d->images, N = I * d->h * d->w, G = (size_t)dt_gplanes(d, op);
  const size_t nseg = ((size_t)d->h + DT_SEG - 1) / DT_SEG;
  size_t o = 0;
  *ws = DtWs{};
  if (d->map_elem == 2) { ws->lab = o; o += dt_align(N); }                    // uint8 [I][h][w]
  ws->g = o;     o += dt_align(G * N * sizeof(uint16_t));                     // [G][I][h][w]
  ws->mask = o;  o += dt_align(G * I * nseg * d->w * sizeof(unsigned long long));   // [G][I][nseg][w]
  ws->flags = o; o += dt_align(G * I * sizeof(unsigned));                     // [G][I]
  ws->total = o;
}

static int dt_check_desc(const OctDtDesc* d, const char* who) {
  OCT_CHECK(d, "%s: null descriptor", who);
  OCT_CHECK(d->classes >= 1 && d->classes <= OCT_MAX_CLASSES, "%s: classes must be 1..%d (got %d)", who, OCT_MAX_CLASSES, d->classes);
  OCT_CHECK(d->images >= 0 && d->h >= 1 && d->w >= 1, "%s: bad geometry %d x %d x %d", who, d->images, d->h, d->w);
  OCT_CHECK(d->h <= DT_MAX_DIM && d->w <= DT_MAX_DIM, "%s: h and w must not exceed %d (got %d x %d)", who, DT_MAX_DIM, d->h, d->w);
  OCT_CHECK((double)d->images * d->h * d->w < 2147483648.0, "%s: images * h * w must stay below 2^31", who);
  OCT_CHECK(d->map_elem == 0 || d->map_elem == 2, "%s: class maps are uint8 (0) or int64 (2), got %d", who, d->map_elem);
  OCT_CHECK(d->op >= OCT_DT_OP_SQUARED && d->op <= OCT_DT_OP_SIGNED, "%s: unknown op %d", who, d->op);
  OCT_CHECK(d->planes >= 1, "%s: the plane list is empty (got %d planes)", who, d->planes);
  OCT_CHECK(d->planes <= OCT_DT_MAX_PLANES, "%s: at most %d planes per call (got %d)", who, OCT_DT_MAX_PLANES, d->planes);
  return OCT_OK;
}

// the label byte of a map value: the class of a valid pixel, DT_NONE otherwise.  Idempotent: the bytes the labels pass wrote
// read back as themselves (with has_ignore = 0)
template <typename T>
__device__ __forceinline__ unsigned dt_code(T raw, int C, int has_ignore, long long ignore_index) {
  const long long v = (long long)raw;
  if (has_ignore && v == ignore_index) return DT_NONE;
  return (unsigned long long)v < (unsigned long long)C ? (unsigned)v : DT_NONE;
}

// ---- labels ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) dt_labels_kernel(const long long* __restrict__ map, uint8_t* __restrict__ lab, size_t npix, int C,
                                                        int has_ignore, long long ignore_index) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  lab[i] = (uint8_t)dt_code(map[i], C, has_ignore, ignore_index);
}

// ---- columns -----------------------------------------------------------------------------------------------------------------
// blockIdx.x = (col * nseg + seg) * strips + strip with col = gplane * images + img; a thread owns one x of the strip
__global__ void __launch_bounds__(256) dt_mask_kernel(const uint8_t* __restrict__ lab, unsigned long long* __restrict__ mask,
                                                      unsigned* __restrict__ flags, const DtPlanes pl, int images, int h, int w, int C,
                                                      int has_ignore, long long ignore_index, int strips, int nseg) {
  const int strip = (int)(blockIdx.x % (unsigned)strips);
  const size_t cs = blockIdx.x / (unsigned)strips;    // col * nseg + seg
  const int seg = (int)(cs % (size_t)nseg);
  const size_t col = cs / (size_t)nseg;
  const int gp = (int)(col / (size_t)images);         // below the plane count: the grid is sized by it
  const size_t img = col % (size_t)images;
  const unsigned kind = pl.kind[gp], c = pl.cls[gp];
  const int x = strip * 256 + (int)threadIdx.x;
  unsigned long long m = 0ull;
  if (x < w) {
    const uint8_t* L = lab + img * (size_t)h * w + x;
    const int y0 = DT_SEG * seg;                       // y0 < h: nseg = ceil(h / DT_SEG)
    const int rows = h - y0 < DT_SEG ? h - y0 : DT_SEG;
#define DT_AT(p) dt_code((p), C, has_ignore, ignore_index)
    if (kind == OCT_DT_BOUNDARY) {
      unsigned prev = y0 > 0 ? DT_AT(L[(size_t)(y0 - 1) * w]) : DT_NONE;
      unsigned cur = DT_AT(L[(size_t)y0 * w]);
      for (int j = 0; j < rows; ++j) {
        const size_t o = (size_t)(y0 + j) * w;
        const unsigned nxt = y0 + j + 1 < h ? DT_AT(L[o + w]) : DT_NONE;
        const unsigned lft = x > 0 ? DT_AT(L[o - 1]) : DT_NONE;
        const unsigned rgt = x + 1 < w ? DT_AT(L[o + 1]) : DT_NONE;
        const bool differs = (prev != DT_NONE && prev != cur) || (nxt != DT_NONE && nxt != cur) || (lft != DT_NONE && lft != cur) ||
                             (rgt != DT_NONE && rgt != cur);
        if (cur != DT_NONE && differs) m |= 1ull << j;
        prev = cur;
        cur = nxt;
      }
    } else {
      const bool other = kind == OCT_DT_OTHER;
#pragma unroll 8
      for (int j = 0; j < rows; ++j) {
        const unsigned v = DT_AT(L[(size_t)(y0 + j) * w]);
        const bool site = other ? (v != DT_NONE && v != c) : v == c;   // c < C: a pixel equal to c is valid
        if (site) m |= 1ull << j;
      }
    }
#undef DT_AT
    mask[cs * (size_t)w + x] = m;
  }
  const unsigned long long any = __ballot(m != 0ull);
  if (any && (threadIdx.x & 63) == 0) atomicOr(&flags[col], 1u);
}

// g[y] = vertical distance to the nearest site of the column (DT_GFAR: none): inside the segment by bit scans of its mask,
// beyond it from the nearest non-empty segment above and below (at most nseg steps each way)
__global__ void __launch_bounds__(256) dt_dist_kernel(const unsigned long long* __restrict__ mask, uint16_t* __restrict__ g, int h, int w,
                                                      int strips, int nseg) {
  const int strip = (int)(blockIdx.x % (unsigned)strips);
  const size_t cs = blockIdx.x / (unsigned)strips;
  const int seg = (int)(cs % (size_t)nseg);
  const size_t col = cs / (size_t)nseg;
  const int x = strip * 256 + (int)threadIdx.x;
  if (x >= w) return;
  const unsigned long long* mc = mask + col * (size_t)nseg * w + x;
  const unsigned long long m = mc[(size_t)seg * w];
  int above = -1, below = -1;                          // rows of the nearest sites outside the segment
  for (int s = seg - 1; s >= 0; --s) {
    const unsigned long long v = mc[(size_t)s * w];
    if (v) { above = DT_SEG * s + 63 - __builtin_clzll(v); break; }
  }
  for (int s = seg + 1; s < nseg; ++s) {
    const unsigned long long v = mc[(size_t)s * w];
    if (v) { below = DT_SEG * s + __builtin_ctzll(v); break; }
  }
  uint16_t* gc = g + col * (size_t)h * w + x;
  const int y0 = DT_SEG * seg;
#pragma unroll 8
  for (int j = 0; j < DT_SEG; ++j) {
    const int y = y0 + j;
    if (y >= h) break;
    const unsigned long long le = m & (~0ull >> (63 - j)), ge = m >> j;
    unsigned up = DT_GFAR, dn = DT_GFAR;
    if (le) up = (unsigned)(j - (63 - __builtin_clzll(le)));
    else if (above >= 0) up = (unsigned)(y - above);
    if (ge) dn = (unsigned)__builtin_ctzll(ge);
    else if (below >= 0) dn = (unsigned)(below - y);
    gc[(size_t)y * w] = (uint16_t)(up < dn ? up : dn);   // a real distance is at most h - 1 < DT_GFAR
  }
}

// ---- rows --------------------------------------------------------------------------------------------------------------------
// A staged g row lies in LDS in blocks of DT_BLK columns, padded to whole blocks, "no site" as DT_LNONE = 2^15 (its square is
// OCT_DT_FAR: such a column never lowers a minimum, and nothing overflows 32 bits); next to it the minimum of every block.
__device__ __forceinline__ void dt_stage(uint16_t* s_g, uint16_t* s_min, const uint16_t* __restrict__ src, int nrows, int w, int stride) {
  const int tid = threadIdx.x, nb = stride / DT_BLK;
  for (int t = tid; t < nrows * stride; t += 256) {
    const int ly = t / stride, x = t - ly * stride;
    unsigned v = DT_LNONE;
    if (x < w) { v = src[ly * w + x]; v = v < DT_LNONE ? v : DT_LNONE; }   // a real g is below 2^14, DT_GFAR becomes DT_LNONE
    s_g[t] = (uint16_t)v;
  }
  __syncthreads();
  for (int b = tid; b < nrows * nb; b += 256) {
    const uint4* q = reinterpret_cast<const uint4*>(s_g + DT_BLK * b);   // 32-byte blocks from a 16-byte aligned base
    const uint4 u0 = q[0], u1 = q[1];
    const unsigned wd[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
    unsigned m = DT_LNONE;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const unsigned lo = wd[i] & 0xFFFFu, hi = wd[i] >> 16;
      m = lo < m ? lo : m;
      m = hi < m ? hi : m;
    }
    s_min[b] = (uint16_t)m;
  }
  __syncthreads();
}

// best = min(best, (x - c)^2 + g[c]^2) over the DT_BLK columns c of one block; d0 = x - (the block's first column)
__device__ __forceinline__ unsigned dt_scan(const uint16_t* blk, int d0, unsigned best) {
  const uint4* q = reinterpret_cast<const uint4*>(blk);
  const uint4 u0 = q[0], u1 = q[1];
  const unsigned wd[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned lo = wd[i] & 0xFFFFu, hi = wd[i] >> 16;
    const int da = d0 - 2 * i, db = da - 1;
    const unsigned va = (unsigned)(da * da) + lo * lo, vb = (unsigned)(db * db) + hi * hi;   // below 2^28 + 2^30
    best = va < best ? va : best;
    best = vb < best ? vb : best;
  }
  return best;
}

// The exact D2 of pixel x of a staged row of nb blocks; OCT_DT_FAR where no column of the row has a site.  First the columns
// x +- r for r < DT_NEAR, ending as soon as r^2 >= best: where sites are dense that is all.  Otherwise the pixel's own block,
// then the blocks j = 1, 2, ... to its left and right while the nearest column of the block, dl or dr away, has d^2 < best; a
// block is scanned only where d^2 + (its smallest g)^2 < best -- every column of it is at least that far.  A side whose d^2 has
// reached best is done for good: d grows and best only falls.  Columns seen twice change nothing.
__device__ __forceinline__ unsigned dt_nearest(const uint16_t* row, const uint16_t* rmin, int x, int nb) {
  unsigned best = OCT_DT_FAR;
#pragma unroll
  for (int r = 0; r < DT_NEAR; ++r) {
    const unsigned rr = (unsigned)(r * r);
    if (rr >= best) return best;
    if (x - r >= 0) { const unsigned gv = row[x - r], v = rr + gv * gv; best = v < best ? v : best; }
    if (r > 0 && x + r < nb * DT_BLK) { const unsigned gv = row[x + r], v = rr + gv * gv; best = v < best ? v : best; }   // padding: DT_LNONE
  }
  if ((unsigned)(DT_NEAR * DT_NEAR) >= best) return best;
  const int kx = x / DT_BLK, xo = x - kx * DT_BLK;
  { const unsigned gm = rmin[kx]; if (gm * gm < best) best = dt_scan(row + DT_BLK * kx, xo, best); }
  for (int j = 1; j < nb; ++j) {
    const int dl = xo + DT_BLK * j - (DT_BLK - 1), dr = DT_BLK * j - xo;   // both >= 1
    const unsigned dl2 = (unsigned)(dl * dl), dr2 = (unsigned)(dr * dr);
    const bool live_l = kx - j >= 0 && dl2 < best, live_r = kx + j < nb && dr2 < best;
    if (!live_l && !live_r) break;
    if (live_l) {
      const unsigned gm = rmin[kx - j];
      if (dl2 + gm * gm < best) best = dt_scan(row + DT_BLK * (kx - j), xo + DT_BLK * j, best);
    }
    if (live_r) {
      const unsigned gm = rmin[kx + j];
      if (dr2 + gm * gm < best) best = dt_scan(row + DT_BLK * (kx + j), xo - DT_BLK * j, best);
    }
  }
  return best;
}

// blockIdx.x = (img * P + p) * groups + grp.  rpw > 1: group grp holds the rows y0 = grp * rpw .. y0 + nrows - 1, n = nrows * w
// contiguous elements of g, of the map and of the output.  rpw == 1: grp = y0 * chunks + chunk, the workgroup holds the whole g
// row (n = w) and answers its pixels t_lo .. t_hi - 1.  LDS: rpw rows of `stride` columns, then rpw * stride / DT_BLK minima
template <int EPI>
__global__ void __launch_bounds__(256) dt_row_kernel(const uint8_t* __restrict__ lab, const uint16_t* __restrict__ g,
                                                     const unsigned* __restrict__ flags, void* __restrict__ out,
                                                     const float* __restrict__ table, unsigned table_last, const DtPlanes pl, int images,
                                                     int h, int w, int P, int C, int has_ignore, long long ignore_index, int rpw,
                                                     int chunks, int groups, int stride) {
  extern __shared__ __attribute__((aligned(16))) uint16_t s_g[];
  uint16_t* s_min = s_g + rpw * stride;
  const int tid = threadIdx.x, nb = stride / DT_BLK;
  const int grp = (int)(blockIdx.x % (unsigned)groups);
  const size_t ip = blockIdx.x / (unsigned)groups;    // img * P + p
  const int p = (int)(ip % (size_t)P);
  const size_t img = ip / (size_t)P;
  const int y0 = rpw > 1 ? grp * rpw : grp / chunks;
  const int nrows = h - y0 < rpw ? h - y0 : rpw;
  const int n = nrows * w;                             // at most max(DT_ROW_PIX, w) <= 16384
  const int t_lo = rpw > 1 ? 0 : (grp % chunks) * DT_ROW_PIX;
  const int t_hi = rpw > 1 || n - t_lo < DT_ROW_PIX ? n : t_lo + DT_ROW_PIX;
  const size_t obase = (ip * h + y0) * (size_t)w;
  if (EPI != DT_EPI_SIGNED) {
    const size_t col = (size_t)p * images + img;
    const bool has = flags[col] != 0u;                 // workgroup-uniform
    if (has) dt_stage(s_g, s_min, g + (col * h + y0) * (size_t)w, nrows, w, stride);
    for (int t = t_lo + tid; t < t_hi; t += 256) {
      unsigned best = OCT_DT_FAR;
      if (has) {
        const int ly = t / w, x = t - ly * w;
        best = dt_nearest(s_g + ly * stride, s_min + ly * nb, x, nb);
      }
      if (EPI == DT_EPI_SQUARED) reinterpret_cast<int*>(out)[obase + t] = (int)best;
      else reinterpret_cast<float*>(out)[obase + t] = table[best < table_last ? best : table_last];   // the index is clamped
    }
  } else {
    // plane p: class c = pl.cls[2p]; g plane 2p holds the distances to class c, 2p + 1 those to the valid pixels outside it
    const unsigned c = pl.cls[2 * p];
    const size_t col_in = (size_t)(2 * p) * images + img, col_out = col_in + images;
    float* o = reinterpret_cast<float*>(out) + obase;
    if (flags[col_in] == 0u || flags[col_out] == 0u) {  // workgroup-uniform: the class is absent, or nothing valid is outside it
      for (int t = t_lo + tid; t < t_hi; t += 256) o[t] = 0.0f;
      return;
    }
    const uint8_t* L = lab + (img * h + y0) * (size_t)w;
#pragma unroll 1
    for (int phase = 0; phase < 2; ++phase) {          // 0: pixels outside the class look for it; 1: its pixels look out of it
      if (phase) __syncthreads();                      // every pixel of phase 0 is answered before its rows are replaced
      dt_stage(s_g, s_min, g + ((phase ? col_out : col_in) * h + y0) * (size_t)w, nrows, w, stride);
      for (int t = t_lo + tid; t < t_hi; t += 256) {
        const bool inside = dt_code(L[t], C, has_ignore, ignore_index) == c;
        if (inside != (phase == 1)) continue;
        const int ly = t / w, x = t - ly * w;
        const float d = sqrtf((float)dt_nearest(s_g + ly * stride, s_min + ly * nb, x, nb));
        o[t] = phase ? -d : d;
      }
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
extern "C" size_t oct_dt_workspace_bytes(const OctDtDesc* d) {
  if (dt_check_desc(d, "oct_dt_workspace_bytes") != OCT_OK) return 0;
  if (d->op == OCT_DT_OP_SIGNED && d->planes > DT_SIGNED_MAX) {
    oct_set_error("oct_dt_workspace_bytes: at most %d classes per signed call (got %d)", DT_SIGNED_MAX, d->planes);
    return 0;
  }
  DtWs ws;
  dt_layout(d, d->op, &ws);
  return ws.total;
}

extern "C" int oct_dt_block(int* rows, int* cols) {
  OCT_CHECK(rows && cols, "oct_dt_block: null output");
  *rows = DT_SEG;
  *cols = DT_ROW_PIX;
  return OCT_OK;
}

// the launches of one call: `pl` names the dt_gplanes(d, op) site sets
static int dt_run(const OctDtDesc* d, int op, const DtPlanes& pl, const void* map, void* out, const float* table, int table_len,
                  void* workspace, void* stream, const char* who) {
  OCT_CHECK(map, "%s: null map", who);
  OCT_CHECK(d->map_elem == 0 || ((uintptr_t)map & 7) == 0, "%s: int64 map not 8-byte aligned", who);
  OCT_CHECK(out && ((uintptr_t)out & 3) == 0, "%s: the output is null or not 4-byte aligned", who);
  OCT_CHECK(workspace && ((uintptr_t)workspace & 15) == 0, "%s: the workspace is null or not 16-byte aligned", who);
  DtWs ws;
  dt_layout(d, op, &ws);
  const int h = d->h, w = d->w, images = d->images, P = d->planes, G = dt_gplanes(d, op);
  const int strips = ceil_div(w, 256), nseg = ceil_div(h, DT_SEG);
  const int rpw = w >= DT_ROW_PIX ? 1 : DT_ROW_PIX / w, chunks = rpw > 1 ? 1 : ceil_div(w, DT_ROW_PIX);
  const int groups = ceil_div(h, rpw) * chunks;
  const size_t sweep_blocks = (size_t)G * images * nseg * strips, row_blocks = (size_t)images * P * groups;
  OCT_CHECK(sweep_blocks < 2147483648ull && row_blocks < 2147483648ull,
            "%s: the batch needs more than 2^31 workgroups: pass fewer images or planes per call", who);
  const size_t npix = (size_t)images * h * w;
  hipStream_t s = as_stream(stream);
  unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
  uint16_t* g = reinterpret_cast<uint16_t*>(base + ws.g);
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(base + ws.mask);
  unsigned* flags = reinterpret_cast<unsigned*>(base + ws.flags);
  const hipError_t e = hipMemsetAsync(flags, 0, (size_t)G * images * sizeof(unsigned), s);
  if (e != hipSuccess) {
    oct_set_error("%s: clearing the site flags failed: %s", who, hipGetErrorString(e));
    return OCT_E_LAUNCH;
  }
  const dim3 b(256);
  const uint8_t* lab = reinterpret_cast<const uint8_t*>(map);
  int has_ignore = d->has_ignore ? 1 : 0;
  const long long ign = (long long)d->ignore_index;
  if (d->map_elem == 2) {                              // narrowed once for all planes; the bytes carry the validity
    uint8_t* narrow = base + ws.lab;
    hipLaunchKernelGGL(dt_labels_kernel, dim3((unsigned)((npix + 255) / 256)), b, 0, s, reinterpret_cast<const long long*>(map), narrow,
                       npix, d->classes, has_ignore, ign);
    lab = narrow;
    has_ignore = 0;
  }
  hipLaunchKernelGGL(dt_mask_kernel, dim3((unsigned)sweep_blocks), b, 0, s, lab, mask, flags, pl, images, h, w, d->classes, has_ignore,
                     ign, strips, nseg);
  hipLaunchKernelGGL(dt_dist_kernel, dim3((unsigned)sweep_blocks), b, 0, s, mask, g, h, w, strips, nseg);
  const int stride = ceil_div(w, DT_BLK) * DT_BLK;    // rpw * stride <= DT_BLK * DT_ROW_PIX = DT_MAX_DIM: w = 1 and w = 16384
  const size_t lds = (((size_t)rpw * stride + (size_t)rpw * (stride / DT_BLK)) * sizeof(uint16_t) + 15) & ~(size_t)15;   // <= 34 KiB
  const dim3 gr((unsigned)row_blocks);
  const unsigned last = table_len > 0 ? (unsigned)(table_len - 1) : 0u;
#define DT_ROWS(EPI)                                                                                                             \
  hipLaunchKernelGGL((dt_row_kernel<EPI>), gr, b, lds, s, lab, g, flags, out, table, last, pl, images, h, w, P, d->classes, has_ignore, \
                     ign, rpw, chunks, groups, stride)
  if (op == OCT_DT_OP_SQUARED) DT_ROWS(DT_EPI_SQUARED);
  else if (op == OCT_DT_OP_WEIGHT) DT_ROWS(DT_EPI_TABLE);
  else DT_ROWS(DT_EPI_SIGNED);
#undef DT_ROWS
  return oct_check_launch(who);
}

// planes: host memory, [planes][2] = (OCT_DT_BOUNDARY / _CLASS / _OTHER, class)
static int dt_planes(const OctDtDesc* d, const int32_t* planes, DtPlanes* pl, const char* who) {
  OCT_CHECK(planes, "%s: null plane list", who);
  *pl = DtPlanes{};
  for (int p = 0; p < d->planes; ++p) {
    const int kind = planes[2 * p], c = planes[2 * p + 1];
    OCT_CHECK(kind >= OCT_DT_BOUNDARY && kind <= OCT_DT_OTHER, "%s: plane %d has unknown kind %d", who, p, kind);
    OCT_CHECK(kind == OCT_DT_BOUNDARY ? c == 0 : (c >= 0 && c < d->classes),
              "%s: plane %d names class %d, the map has classes 0..%d (a boundary plane takes 0)", who, p, c, d->classes - 1);
    pl->kind[p] = (uint8_t)kind;
    pl->cls[p] = (uint8_t)c;
  }
  return OCT_OK;
}

extern "C" int oct_dt_squared(const OctDtDesc* d, const int32_t* planes, const void* map, int32_t* out, void* workspace, void* stream) {
  int rc = dt_check_desc(d, "oct_dt_squared");
  if (rc != OCT_OK) return rc;
  DtPlanes pl;
  if ((rc = dt_planes(d, planes, &pl, "oct_dt_squared")) != OCT_OK) return rc;
  if (d->images == 0) return OCT_OK;
  return dt_run(d, OCT_DT_OP_SQUARED, pl, map, out, nullptr, 0, workspace, stream, "oct_dt_squared");
}

extern "C" int oct_dt_weight_map(const OctDtDesc* d, const int32_t* planes, const void* map, const float* table, int table_len,
                                 float* out, void* workspace, void* stream) {
  int rc = dt_check_desc(d, "oct_dt_weight_map");
  if (rc != OCT_OK) return rc;
  DtPlanes pl;
  if ((rc = dt_planes(d, planes, &pl, "oct_dt_weight_map")) != OCT_OK) return rc;
  OCT_CHECK(table_len >= 1, "oct_dt_weight_map: the table is empty (got %d entries)", table_len);
  if (d->images == 0) return OCT_OK;
  OCT_CHECK(table && ((uintptr_t)table & 3) == 0, "oct_dt_weight_map: the table is null or not 4-byte aligned");
  return dt_run(d, OCT_DT_OP_WEIGHT, pl, map, out, table, table_len, workspace, stream, "oct_dt_weight_map");
}

extern "C" int oct_dt_signed(const OctDtDesc* d, const int32_t* class_ids, const void* map, float* out, void* workspace, void* stream) {
  int rc = dt_check_desc(d, "oct_dt_signed");
  if (rc != OCT_OK) return rc;
  OCT_CHECK(d->planes <= DT_SIGNED_MAX, "oct_dt_signed: at most %d classes per call (got %d)", DT_SIGNED_MAX, d->planes);
  OCT_CHECK(class_ids, "oct_dt_signed: null class list");
  DtPlanes pl = {};
  for (int k = 0; k < d->planes; ++k) {
    const int c = class_ids[k];
    OCT_CHECK(c >= 0 && c < d->classes, "oct_dt_signed: entry %d names class %d, the map has classes 0..%d", k, c, d->classes - 1);
    pl.kind[2 * k] = OCT_DT_CLASS;
    pl.kind[2 * k + 1] = OCT_DT_OTHER;
    pl.cls[2 * k] = pl.cls[2 * k + 1] = (uint8_t)c;
  }
  if (d->images == 0) return OCT_OK;
  return dt_run(d, OCT_DT_OP_SIGNED, pl, map, out, nullptr, 0, workspace, stream, "oct_dt_signed");
}
