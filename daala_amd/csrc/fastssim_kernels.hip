/* fastssim_kernels.hip - FastSSIM on the device, as the reference's RD tool computes it (calc_ssim :445-463 of
   tools/dump_fastssim.c, with fs_downsample_level0 :148-190, fs_calc_structure :318-418, fs_apply_luminance :192-256).

   Four levels of a w x h plane pair.  Level 0 is the 2x2 SUM of the pair at ceil(w/2) x ceil(h/2), a missing right or
   bottom neighbour replaced by the last sample; level l > 0 the 2x2 sum of level l - 1 at the rounded-up size, clamped
   the same way AT THAT LEVEL'S OWN LAST ROW AND COLUMN.  (The tool clamps levels 1..3 one past the last row and column
   - a defect: it reads the next row's first sample, or a row of another array.  It is not copied; the library equals
   the tool where the tool's reads stay inside, see odhip_fastssim_tool_exact in daala_hip.h.)

   At every level the gradient magnitudes g = 4 max(g1, g2) + min(g1, g2) of the two diagonal differences on the
   (w_l - 1) x (h_l - 1) interior, zero outside; three sums of gx^2, gy^2 and gx gy under the fixed 8 x 8 integer window
   kTable (total 104; what the tool's sliding scheme of doubling, halving and subtracting columns amounts to:
   tests/_fastssim_ref.py ports those loops and compares); the term (2 mugxgy + c2)/(mugx2 + mugy2 + c2).
   Exactness: a sample of level l is at most max 4^(l + 1), 4095 * 256 < 2^20 at 12 bits and level 3; a difference is
   at most that, g <= 5 * 4095 * 256 < 2^22.33 (uint32), g^2 < 2^44.65 and 104 g^2 < 2^51.36 < 2^52 - for samples within
   the depth: ODHIP_SAMPLE_U16 planes are read as they are, and a value above (1 << depth) - 1 voids the bound, as it
   voids max.  So the three sums
   are mathematical integers that int64 holds and that convert to double without rounding - and the tool's doubles,
   partial sums (halves included) below 2^52 throughout, are the same integers whatever its order of summation.
   Level 3 multiplies in the luminance term over 8 x 8 BOX sums mux, muy (rows j - 4 .. j + 3, columns i - 4 .. i + 3,
   coordinates clamped to the level), held as the tool holds them in `unsigned`; the tool slides muy along a row with
   x's column sums (:243-244), so muy(j, i) = muy(j, 0) + mux(j, i) - mux(j, 0) modulo 2^32.  c1 and c2 come from the
   host, evaluated in the tool's association.

   k_fastssim_pyramid  one workgroup per 64x64 samples of a plane in any ODHIP_SAMPLE_* format: the 32x32 sums of level
                       0 from global memory, 16x16 / 8x8 / 4x4 of levels 1..3 from LDS; all four written as int32.  A
                       flat grid over the planes of a launch group: every reconstruction and every DISTINCT source.
   k_fastssim          one workgroup per 32x32 output tile of one level of a pair (a flat grid over pairs, levels and
                       tiles).  Both planes' samples of rows R - 4 .. R + 36 and columns C - 4 .. C + 35 around the tile
                       at (R, C) are staged in LDS with clamped coordinates (rows R - 3 .. R + 36 feed the gradients,
                       row R - 4 only the box sums); gx and gy of rows R - 3 .. R + 35 and columns C - 4 .. C + 34 are
                       written once as uint32, zero outside the gradient domain.  A lane owns one column and four
                       consecutive rows of the tile: it reads each of its 11 x 8 gradient pairs once, forms the three
                       products with 32 x 32 + 64 bit multiply-adds and folds them into the row's sums under the table's
                       four row classes - the weights are powers of two, so a class is the class before shifted once
                       plus two products - which its four outputs add into int64 registers: the 44 taps of the table
                       exactly, at 24 multiplies and 9 shifts per gradient row instead of 132 per output.  The term is
                       formed in double (__ddiv_rn, -ffp-contract=off).  At level 3 the box sums come from the staged
                       samples; mux(j, 0) and muy(j, 0) of the tile's 32 rows are RECOMPUTED from the level in global
                       memory (8 x 4 samples per row start and plane, the first 32 lanes; level 3 is 1/256 of the
                       plane, no pre-pass is worth a launch).  The lane adds its four terms in row order, the workgroup
                       reduces in a fixed tree and leaves one partial per tile.
   The launch groups, their planes and scratch, and k_metric_tile_sum, which adds the partials of a (pair, level) in a
   fixed order -> sums[pair][level], are od_metric_launch.cuh's.
   LDS of k_fastssim: 2 x 41 x 40 x 4 B samples + 2 x 39 x 40 x 4 B gradients + 2 KiB reduction + 256 B = 27.3 KiB. */
#include <math.h>
#include <string.h>
#include "../../include/daala_hip.h"
#include "od_ctx.cuh"
#include "od_metric_launch.cuh"
#include "od_sample.cuh"

namespace {

constexpr int kLevels = ODHIP_FASTSSIM_LEVELS;
constexpr int kMinSize = 16;                          /* as the other pyramid metric: level 3 of 16 x 16 is 1 x 1 */
constexpr int kOwn = 4;                               /* consecutive rows of a lane: it owns 1 column x 4 rows */
constexpr int kWin = 8;                               /* the window and the box */
constexpr int kGradRows = kTile + kWin - 1;           /* gradient rows R - 3 .. R + 35 */
constexpr int kGradCols = kTile + kWin - 1;           /* gradient columns C - 4 .. C + 34 */
constexpr int kRowsS = kGradRows + 2;                 /* sample rows R - 4 .. R + 36 */
constexpr int kPitch = kGradCols + 1;                 /* sample columns C - 4 .. C + 35; the gradients' pitch too */
constexpr int kPyrTile = kTile;                       /* k_fastssim_pyramid: 32 x 32 sums of level 0 per workgroup */
static_assert(kThreads*kOwn == kTile*kTile, "k_fastssim: a lane owns kOwn samples of the tile");

/* log2 of the window's weights, -1 where it is zero.  An impulse at gradient position (y, x) lands on output rows
   y - 4 .. y + 3 and columns x - 3 .. x + 4 with these weights:
     out(r, c) = sum over a, b of (1 << kTable[a][b]) * G(r + 4 - a, c + 3 - b) */
struct FsTable {
  int s[kWin][kWin];
};
constexpr FsTable kTable = {{
 {0, 1, 2, 3, 3, 2, 1, 0},
 {0, 1, 2, 3, 3, 2, 1, 0},
 {-1, 0, 1, 2, 2, 1, 0, -1},
 {-1, -1, 0, 1, 1, 0, -1, -1},
 {-1, -1, -1, 0, 0, -1, -1, -1},
 {-1, -1, -1, 0, 0, -1, -1, -1},
 {-1, -1, 0, 1, 1, 0, -1, -1},
 {-1, 0, 1, 2, 2, 1, 0, -1}}};

constexpr int table_weight() {
  int sum = 0;
  for (int a = 0; a < kWin; a++) {
    for (int b = 0; b < kWin; b++) sum += kTable.s[a][b] < 0 ? 0 : 1 << kTable.s[a][b];
  }
  return sum;
}
static_assert(table_weight() == 104, "the window the tool's sliding loops give on unit impulses: total weight 104");

/* The table's rows come in four classes, each the one before doubled plus one more pair of columns:
     class 0: 0 0 0 1 1 0 0 0   class 1: 0 0 1 2 2 1 0 0   class 2: 0 1 2 4 4 2 1 0   class 3: 1 2 4 8 8 4 2 1 */
struct FsRowClass {
  int s[kWin];
};
constexpr FsRowClass kRowClass = {{3, 3, 2, 1, 0, 0, 1, 2}};

constexpr bool classes_are_the_table() {
  for (int a = 0; a < kWin; a++) {
    for (int b = 0; b < kWin; b++) {
      /* column b of class c: 1 << (c - distance from the two middle columns), zero where that is negative */
      const int sh = kRowClass.s[a] - (b < 4 ? 3 - b : b - 4);
      if ((sh < 0 ? -1 : sh) != kTable.s[a][b]) return false;
    }
  }
  return true;
}
static_assert(classes_are_the_table(), "row_sums folds exactly kTable");

/* h[c] = the sum over b of (class c's weight of column b) * p[b]*q[b], one 32 x 32 + 64 bit multiply-add per product;
   the weights are powers of two, so a class is the class before shifted once plus two products (8 * 8 g^2 < 2^52) */
__device__ __forceinline__ void row_sums(const uint32_t (&p)[kWin], const uint32_t (&q)[kWin], uint64_t (&h)[4]) {
  h[0] = (uint64_t)p[3]*q[3] + (uint64_t)p[4]*q[4];
#pragma unroll
  for (int c = 1; c < 4; c++) h[c] = (h[c - 1] << 1) + (uint64_t)p[3 - c]*q[3 - c] + (uint64_t)p[4 + c]*q[4 + c];
}

/* the size of level l along an axis of n samples: l + 1 halvings, each rounded up */
__host__ __device__ inline int level_dim(int n, int l) {
  return (n + (1 << (l + 1)) - 1) >> (l + 1);
}

/* elements of levels 0 .. l - 1 of a w x h plane's pyramid: where level l starts; l = kLevels: the whole pyramid */
__host__ __device__ inline size_t pyr_offset(int w, int h, int l) {
  size_t o = 0;
  for (int i = 0; i < l; i++) o += (size_t)level_dim(w, i)*(size_t)level_dim(h, i);
  return o;
}

struct FsBatch {
  MetricGroup g;                                      /* a column is a level */
  int w[kBatch], h[kBatch];
  int dsel[kBatch];                                   /* (depth - 8)/2: the pair's row of c1 and c2 */
  double c2[3][kLevels];
  double c1[3];                                       /* level 3's */
};

/* the 2x2 sum at (lx, ly) of an LDS level whose sample (0, 0) is sample (x0, y0) of a wl x hl level; x0, y0 even, so
   the left and upper samples are inside the tile and the clamp only ever folds the neighbour back onto them */
template <int N>
__device__ __forceinline__ int down_lds(const int32_t (&s)[N][N], int lx, int ly, int x0, int y0, int wl, int hl) {
  const int xa = 2*lx;
  const int ya = 2*ly;
  const int xb = x0 + xa + 1 < wl ? xa + 1 : xa;
  const int yb = y0 + ya + 1 < hl ? ya + 1 : ya;
  return s[ya][xa] + s[ya][xb] + s[yb][xa] + s[yb][xb];
}

__global__ __launch_bounds__(kThreads) void k_fastssim_pyramid(MetricPyrBatch b, int nplanes, int32_t *pyr) {
  __shared__ int32_t s0[kPyrTile][kPyrTile];
  __shared__ int32_t s1[kPyrTile/2][kPyrTile/2];
  __shared__ int32_t s2[kPyrTile/4][kPyrTile/4];
  const int tid = threadIdx.x;
  const int pi = find_entry(b.block0, nplanes, (int)blockIdx.x);
  const MetricPlane &q = b.pl[pi];
  int wl[kLevels], hl[kLevels];
#pragma unroll
  for (int l = 0; l < kLevels; l++) {
    wl[l] = level_dim(q.w, l);
    hl[l] = level_dim(q.h, l);
  }
  const int nbx = (wl[0] + kPyrTile - 1)/kPyrTile;
  const int t = (int)blockIdx.x - b.block0[pi];
  const int bx = (t%nbx)*kPyrTile;                    /* in samples of level 0 */
  const int by = (t/nbx)*kPyrTile;
  int32_t *o0 = pyr + q.pyr;
  int32_t *o1 = o0 + pyr_offset(q.w, q.h, 1);
  int32_t *o2 = o0 + pyr_offset(q.w, q.h, 2);
  int32_t *o3 = o0 + pyr_offset(q.w, q.h, 3);
#pragma unroll
  for (int j = 0; j < kPyrTile*kPyrTile/kThreads; j++) {
    const int i = tid + kThreads*j;
    const int lx = i%kPyrTile;
    const int ly = i/kPyrTile;
    const int x = bx + lx;
    const int y = by + ly;
    int v = 0;
    if (x < wl[0] && y < hl[0]) {
      /* 2x <= w - 1 and 2y <= h - 1; the neighbours fold back onto the last column and row (:165, :170) */
      const int x1 = min(2*x + 1, q.w - 1);
      const int y1 = min(2*y + 1, q.h - 1);
      v = load_sample(q.base, q.fmt, q.stride, 2*x, 2*y, q.depth) + load_sample(q.base, q.fmt, q.stride, x1, 2*y, q.depth)
       + load_sample(q.base, q.fmt, q.stride, 2*x, y1, q.depth) + load_sample(q.base, q.fmt, q.stride, x1, y1, q.depth);
      o0[(size_t)y*wl[0] + x] = v;
    }
    s0[ly][lx] = v;
  }
  __syncthreads();
  /* a sample of level l + 1 inside its plane reads only samples of level l inside theirs */
  {
    const int lx = tid%(kPyrTile/2);
    const int ly = tid/(kPyrTile/2);
    const int x = bx/2 + lx;
    const int y = by/2 + ly;
    int v = 0;
    if (x < wl[1] && y < hl[1]) {
      v = down_lds(s0, lx, ly, bx, by, wl[0], hl[0]);
      o1[(size_t)y*wl[1] + x] = v;
    }
    s1[ly][lx] = v;
  }
  __syncthreads();
  if (tid < (kPyrTile/4)*(kPyrTile/4)) {
    const int lx = tid%(kPyrTile/4);
    const int ly = tid/(kPyrTile/4);
    const int x = bx/4 + lx;
    const int y = by/4 + ly;
    int v = 0;
    if (x < wl[2] && y < hl[2]) {
      v = down_lds(s1, lx, ly, bx/2, by/2, wl[1], hl[1]);
      o2[(size_t)y*wl[2] + x] = v;
    }
    s2[ly][lx] = v;
  }
  __syncthreads();
  if (tid < (kPyrTile/8)*(kPyrTile/8)) {
    const int lx = tid%(kPyrTile/8);
    const int ly = tid/(kPyrTile/8);
    const int x = bx/8 + lx;
    const int y = by/8 + ly;
    if (x < wl[3] && y < hl[3]) o3[(size_t)y*wl[3] + x] = down_lds(s2, lx, ly, bx/4, by/4, wl[2], hl[2]);
  }
}

/* |a - d| and |b - c| of a 2x2 neighbourhood a b / c d -> 4 max + min (:354-356) */
__device__ __forceinline__ uint32_t grad(int a, int bq, int c, int d) {
  const uint32_t g1 = (uint32_t)abs(d - a);
  const uint32_t g2 = (uint32_t)abs(c - bq);
  return 4*max(g1, g2) + min(g1, g2);
}

__global__ __launch_bounds__(kThreads) void k_fastssim(FsBatch b, const int32_t *pyr, double *part, double *terms) {
  __shared__ int32_t sx[kRowsS][kPitch];
  __shared__ int32_t sy[kRowsS][kPitch];
  __shared__ uint32_t gx[kGradRows][kPitch];
  __shared__ uint32_t gy[kGradRows][kPitch];
  __shared__ uint32_t x0s[kTile];
  __shared__ uint32_t y0s[kTile];
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  const int e = find_entry(b.g.t.first, b.g.n*kLevels, (int)blockIdx.x);
  const int pi = e/kLevels;
  const int lv = e%kLevels;
  const int w = level_dim(b.w[pi], lv);
  const int h = level_dim(b.h[pi], lv);
  const int t = (int)blockIdx.x - b.g.t.first[e];
  const int ntx = (w + kTile - 1)/kTile;
  const int tx0 = (t%ntx)*kTile;
  const int ty0 = (t/ntx)*kTile;
  const int32_t *ps = pyr + b.g.spyr[pi] + pyr_offset(b.w[pi], b.h[pi], lv);
  const int32_t *pr = pyr + b.g.rpyr[pi] + pyr_offset(b.w[pi], b.h[pi], lv);
  /* staged sample (r, c) is sample (ty0 - 4 + r, tx0 - 4 + c) of the level, coordinates clamped: every read is inside
     the level, and the box sums find their replicated edges in place */
  for (int i = tid; i < kRowsS*kPitch; i += kThreads) {
    const int r = i/kPitch;
    const int c = i - r*kPitch;
    const int y = min(max(ty0 - 4 + r, 0), h - 1);
    const int x = min(max(tx0 - 4 + c, 0), w - 1);
    const size_t at = (size_t)y*w + x;
    sx[r][c] = ps[at];
    sy[r][c] = pr[at];
  }
  if (lv == kLevels - 1 && tid < kTile) {
    /* mux(j, 0) and muy(j, 0) of the tile's row tid, from the level: column 0 five times, then columns 1, 2, 3 */
    const int j = ty0 + tid;
    uint32_t mx = 0, my = 0;
    if (j < h) {
      for (int dj = -4; dj < 4; dj++) {
        const size_t row = (size_t)min(max(j + dj, 0), h - 1)*w;
        mx += 5u*(uint32_t)ps[row];
        my += 5u*(uint32_t)pr[row];
        for (int i = 1; i < 4; i++) {
          mx += (uint32_t)ps[row + min(i, w - 1)];
          my += (uint32_t)pr[row + min(i, w - 1)];
        }
      }
    }
    x0s[tid] = mx;
    y0s[tid] = my;
  }
  __syncthreads();
  /* gradient (r, c) is gradient (ty0 - 3 + r, tx0 - 4 + c) of the level: staged samples (r + 1 .. r + 2, c .. c + 1);
     zero outside the (h - 1) x (w - 1) interior, where the tool's buffers hold zeros - never clamped */
  for (int i = tid; i < kGradRows*kGradCols; i += kThreads) {
    const int r = i/kGradCols;
    const int c = i - r*kGradCols;
    const int y = ty0 - 3 + r;
    const int x = tx0 - 4 + c;
    uint32_t vx = 0, vy = 0;
    if (y >= 0 && y < h - 1 && x >= 0 && x < w - 1) {
      vx = grad(sx[r + 1][c], sx[r + 1][c + 1], sx[r + 2][c], sx[r + 2][c + 1]);
      vy = grad(sy[r + 1][c], sy[r + 1][c + 1], sy[r + 2][c], sy[r + 2][c + 1]);
    }
    gx[r][c] = vx;
    gy[r][c] = vy;
  }
  __syncthreads();
  const int ox = tid%kTile;
  const int oy = kOwn*(tid/kTile);
  const int x = tx0 + ox;
  double sum = 0;
  if (x < w && ty0 + oy < h) {
    /* output row oy + j takes gradient row oy + j + 7 - a and column ox + 7 - b at weight kTable[a][b]: a gradient
       row's eight products are folded once into its four row sums (row_sums) and shared by the lane's four outputs */
    uint64_t x2[kOwn] = {}, y2[kOwn] = {}, xy[kOwn] = {};
#pragma unroll
    for (int gr = 0; gr < kOwn + kWin - 1; gr++) {
      uint32_t vx[kWin], vy[kWin];
#pragma unroll
      for (int bb = 0; bb < kWin; bb++) {
        vx[bb] = gx[oy + gr][ox + 7 - bb];
        vy[bb] = gy[oy + gr][ox + 7 - bb];
      }
      uint64_t hx[4], hy[4], hxy[4];
      row_sums(vx, vx, hx);
      row_sums(vy, vy, hy);
      row_sums(vx, vy, hxy);
#pragma unroll
      for (int j = 0; j < kOwn; j++) {
        const int a = j + 7 - gr;
        if (a < 0 || a >= kWin) continue;
        x2[j] += hx[kRowClass.s[a]];
        y2[j] += hy[kRowClass.s[a]];
        xy[j] += hxy[kRowClass.s[a]];
      }
    }
    const double c2 = b.c2[b.dsel[pi]][lv];
    const double c1 = b.c1[b.dsel[pi]];
#pragma unroll
    for (int j = 0; j < kOwn; j++) {
      const int y = ty0 + oy + j;
      if (y >= h) break;
      /* :392, operation by operation; the three conversions are exact */
      double term = __ddiv_rn(2*(double)(int64_t)xy[j] + c2, (double)(int64_t)x2[j] + (double)(int64_t)y2[j] + c2);
      if (lv == kLevels - 1) {
        uint32_t mux = 0;
#pragma unroll
        for (int r = 0; r < kWin; r++) {
#pragma unroll
          for (int c = 0; c < kWin; c++) mux += (uint32_t)sx[oy + j + r][ox + c];
        }
        /* :231-245: muy starts a row as y's box sum and then moves by x's differences, modulo 2^32: the
           reconstruction's samples beyond column 3 never reach it */
        const uint32_t muy = y0s[oy + j] + mux - x0s[oy + j];
        const double dx = (double)mux;
        const double dy = (double)muy;
        /* :239; 2*mux is the tool's unsigned product */
        term = term*__ddiv_rn((double)(2u*mux)*dy + c1, dx*dx + dy*dy + c1);
      }
      if (terms) terms[(size_t)y*w + x] = term;
      sum += term;
    }
  }
  red[tid] = sum;
  __syncthreads();
  for (int s = kThreads/2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = red[0];
}

bool size_ok(int w, int h) {
  return w >= kMinSize && h >= kMinSize && w <= 65535 && h <= 65535;
}

bool fs_pair_ok(const odhip_metrics_pair &q) {
  return pair_ok(q) && size_ok(q.w, q.h);
}

struct FsTraits {
  static constexpr int kLevels = ODHIP_FASTSSIM_LEVELS;
  static size_t pyr_elems(int w, int h) { return pyr_offset(w, h, kLevels); }
  static long pyr_blocks(int w, int h) {
    return (long)((level_dim(w, 0) + kPyrTile - 1)/kPyrTile)*((level_dim(h, 0) + kPyrTile - 1)/kPyrTile);
  }
  static long tiles(int w, int h, int l) {
    return (long)((level_dim(w, l) + kTile - 1)/kTile)*((level_dim(h, l) + kTile - 1)/kTile);
  }
};

/* One launch group (metric_launch_build); only_level >= 0: that level alone, its terms go to `terms`. */
int fs_launch(MetricScratch *st, const odhip_metrics_pair *pairs, const int *idx, int m, int only_level, double *d_sums,
 double *terms, hipStream_t s) {
  MetricLaunch L;
  const int rc = metric_launch_build<FsTraits>(&L, st, pairs, idx, m, only_level, s);
  if (rc) return rc;
  FsBatch b;
  memset(&b, 0, sizeof(b));
  b.g = L.g;
  for (int i = 0; i < m; i++) {
    const odhip_metrics_pair &q = pairs[idx[i]];
    b.w[i] = q.w;
    b.h[i] = q.h;
    b.dsel[i] = (q.depth - 8)/2;
  }
  for (int d = 0; d < 3; d++) {
    /* :225 and :346, in the tool's association */
    const int samplemax = (1 << (8 + 2*d)) - 1;
    for (int l = 0; l < kLevels; l++) b.c2[d][l] = samplemax*samplemax*(0.03*0.03)*(1 << 4*l)*16*104;
    b.c1[d] = (double)(samplemax*samplemax*(0.01*0.01)*4096*(1 << 4*(kLevels - 1)));
  }
  k_fastssim_pyramid<<<(unsigned)L.blocks, kThreads, 0, s>>>(L.pb, L.nplanes, st->pyr.p);
  k_fastssim<<<(unsigned)L.tiles, kThreads, 0, s>>>(b, st->pyr.p, st->part.p, terms);
  if (d_sums) metric_tile_sum(b.g.t, m, st->part.p, d_sums, s);
  return ODHIP_SUCCESS;
}

}  // namespace

extern "C" int odhip_fastssim_level_size(int w, int h, int level, int *wl, int *hl) {
  if (!size_ok(w, h) || level < 0 || level >= kLevels || !wl || !hl) return ODHIP_EINVAL;
  *wl = level_dim(w, level);
  *hl = level_dim(h, level);
  return ODHIP_SUCCESS;
}

/* 1 where fs_downsample_level's neighbours (:134, :139) stay inside the level they are read from: levels 0, 1 and 2
   even in both directions, so that no neighbour is ever missing */
extern "C" int odhip_fastssim_tool_exact(int w, int h) {
  if (!size_ok(w, h)) return ODHIP_EINVAL;
  for (int l = 0; l < kLevels - 1; l++) {
    if ((level_dim(w, l) | level_dim(h, l)) & 1) return 0;
  }
  return 1;
}

/* calc_ssim's product (:450-460 with fs_average :430-443) with the host libm's pow: a negative sum gives NAN there too */
extern "C" int odhip_fastssim_score(const double sums[4], int w, int h, double *score) {
  static const double kWeight[kLevels] = {0.2989654541015625, 0.3141326904296875, 0.2473602294921875, 0.1395416259765625};
  if (!sums || !score || !size_ok(w, h)) return ODHIP_EINVAL;
  double ret = 1;
  for (int l = 0; l < kLevels; l++) ret *= pow(sums[l]/(level_dim(w, l)*level_dim(h, l)), kWeight[l]);
  *score = ret;
  return ODHIP_SUCCESS;
}

extern "C" int odhip_fastssim_prepare(int w, int h, int pairs) {
  if (!size_ok(w, h) || pairs < 1) return ODHIP_EINVAL;
  ODHIP_CTX_OR_RETURN(ctx);
  return metric_prepare<FsTraits>(odhip_ctx_state<MetricScratch>(ctx, ODHIP_SLOT_FASTSSIM), w, h, pairs);
}

extern "C" int odhip_fastssim_planes(const odhip_metrics_pair *pairs, int n, double *d_sums, odhip_stream stream) {
  if (n < 0 || !pairs || !d_sums) return ODHIP_EINVAL;
  for (int i = 0; i < n; i++) {
    if (!fs_pair_ok(pairs[i])) return ODHIP_EINVAL;
  }
  if (n == 0) return ODHIP_SUCCESS;
  ODHIP_CTX_OR_RETURN(ctx);
  MetricScratch *st = odhip_ctx_state<MetricScratch>(ctx, ODHIP_SLOT_FASTSSIM);
  const int rc = metric_planes<FsTraits>(pairs, n, [&](const int *idx, int m) {
    return fs_launch(st, pairs, idx, m, -1, d_sums, nullptr, (hipStream_t)stream);
  });
  return rc ? rc : odhip_check_launch();
}

extern "C" int odhip_fastssim_terms(const odhip_metrics_pair *pair, int level, double *d_terms, odhip_stream stream) {
  if (!pair || !d_terms || level < 0 || level >= kLevels || !fs_pair_ok(*pair)) return ODHIP_EINVAL;
  ODHIP_CTX_OR_RETURN(ctx);
  const int idx = 0;
  const int rc = fs_launch(odhip_ctx_state<MetricScratch>(ctx, ODHIP_SLOT_FASTSSIM), pair, &idx, 1, level, nullptr,
   d_terms, (hipStream_t)stream);
  return rc ? rc : odhip_check_launch();
}
