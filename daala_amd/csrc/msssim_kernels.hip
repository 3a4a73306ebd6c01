/* msssim_kernels.hip - MS-SSIM on the device, as the reference's RD tool computes it (calc_msssim :228-273 and
   calc_ssim :88-195 of tools/dump_msssim.c).

   Five scales of a w x h plane pair: scale 0 is the pair, scale i > 0 the 2x2 SUM of scale i - 1 at (w >> 1) x
   (h >> 1) (an odd last row or column dropped), `max` - (1 << depth) - 1 at scale 0 - times 4.  At every scale the
   nine taps of gaussian_filter_init(1.5, 5) at weight 1024 run along the rows, then down the columns, over the
   moments mux, muy, x2, xy, y2 and the weight w; taps outside the plane are dropped (the halo is clipped, never
   clamped or mirrored).  The taps are a compile-time table (each lies at least 0.28 from a rounding boundary);
   odhip_msssim_taps rebuilds them with the host libm as the tool does and compares the two.

   k_msssim_pyramid  one workgroup per 64x64 samples of a plane in any ODHIP_SAMPLE_* format: the 32x32 sums of
                     scale 1 from global memory, scales 2..4 from LDS; all four written as int32 (a scale-4 sum of
                     12-bit samples is below 2^20).  A flat grid over the planes of a launch group: every
                     reconstruction and every DISTINCT source plane (the levels of a pipe step share theirs).
   k_msssim          one workgroup per 32x32 output tile of one scale of a pair (a flat grid over pairs, scales and
                     tiles).  The tile and a halo of 4, clipped at the plane, are staged in LDS as int32; the
                     horizontal moments of eight staged rows at a time go through LDS as int64 (1024 x (2^20)^2 =
                     2^50 at scale 4; 2^34 at scale 0 of 12 bits); a lane owns one column and four rows of the tile
                     and adds tap x moment into int64 registers (below 2^61).  The weight is separable (row sum x
                     column sum).  Each sample's cs and ssim are the tool's double expressions, one IEEE operation
                     per C operation in its association (-ffp-contract=off); a moment above 2^53 enters through the
                     int64 -> double conversion, which rounds to nearest.  The lane adds its four terms (cs at
                     scales 0..3, ssim at scale 4) in row order, the workgroup reduces in a fixed tree and leaves
                     one partial per tile.
   The launch groups, their planes and scratch, and k_metric_tile_sum, which adds the partials of a (pair, scale) in a
   fixed order -> sums[pair][scale], are od_metric_launch.cuh's.
   LDS of k_msssim: 2 x 40 x 40 x 4 B samples + 5 x 8 x 32 x 8 B moments + 2 KiB reduction = 25 KiB. */
#include <math.h>
#include <string.h>
#include <algorithm>
#include "../../include/daala_hip.h"
#include "od_ctx.cuh"
#include "od_metric_launch.cuh"
#include "od_sample.cuh"

namespace {

constexpr int kScales = ODHIP_MSSSIM_SCALES;
constexpr int kRadius = 4;
constexpr int kTaps = 2*kRadius + 1;
constexpr int kMinSize = ODHIP_MSSSIM_MIN_SIZE;       /* scale 4 of 16 x 16 is 1 x 1 */
constexpr int kSpan = kTile + 2*kRadius;              /* the tile with its halo */
constexpr int kRows = 8;                              /* staged rows whose horizontal moments are in LDS at a time */
constexpr int kPyrTile = kTile;                       /* k_msssim_pyramid: 32 x 32 sums of scale 1 per workgroup */
/* a lane owns 1 column x 4 rows of the tile */
static_assert(kThreads == kTile*kRows, "k_msssim: one horizontal moment set per lane and row group");

/* the one table: the host's weights, the unrolled horizontal pass and (through kTapDev and LDS) the vertical pass */
struct MsTaps {
  int t[kTaps];
};
constexpr MsTaps kTapTable = {{8, 37, 112, 218, 274, 218, 112, 37, 8}};
__constant__ MsTaps kTapDev = kTapTable;

/* elements of scales 1 .. s - 1 of a w x h plane's pyramid: where scale s starts; s = kScales: the whole pyramid */
__host__ __device__ inline size_t pyr_offset(int w, int h, int s) {
  size_t o = 0;
  for (int i = 1; i < s; i++) o += (size_t)(w >> i)*(size_t)(h >> i);
  return o;
}

struct MsBatch {
  odhip_metrics_pair p[kBatch];
  MetricGroup g;                                      /* a column is a scale */
};

__global__ __launch_bounds__(kThreads) void k_msssim_pyramid(MetricPyrBatch b, int nplanes, int32_t *pyr) {
  __shared__ int32_t s1[kPyrTile][kPyrTile];
  __shared__ int32_t s2[kPyrTile/2][kPyrTile/2];
  __shared__ int32_t s3[kPyrTile/4][kPyrTile/4];
  const int tid = threadIdx.x;
  const int pi = find_entry(b.block0, nplanes, (int)blockIdx.x);
  const MetricPlane &q = b.pl[pi];
  const int w1 = q.w >> 1, h1 = q.h >> 1;
  const int nbx = (w1 + kPyrTile - 1)/kPyrTile;
  const int t = (int)blockIdx.x - b.block0[pi];
  const int bx = (t%nbx)*kPyrTile;                    /* in samples of scale 1 */
  const int by = (t/nbx)*kPyrTile;
  int32_t *o1 = pyr + q.pyr;
  int32_t *o2 = o1 + pyr_offset(q.w, q.h, 2);
  int32_t *o3 = o1 + pyr_offset(q.w, q.h, 3);
  int32_t *o4 = o1 + pyr_offset(q.w, q.h, 4);
#pragma unroll
  for (int j = 0; j < kPyrTile*kPyrTile/kThreads; j++) {
    const int i = tid + kThreads*j;
    const int lx = i%kPyrTile;
    const int ly = i/kPyrTile;
    const int x = bx + lx;
    const int y = by + ly;
    int v = 0;
    if (x < w1 && y < h1) {
      /* 2x + 1 < w and 2y + 1 < h: the odd last column and row are never read */
      v = load_sample(q.base, q.fmt, q.stride, 2*x, 2*y, q.depth) + load_sample(q.base, q.fmt, q.stride, 2*x + 1, 2*y, q.depth)
       + load_sample(q.base, q.fmt, q.stride, 2*x, 2*y + 1, q.depth)
       + load_sample(q.base, q.fmt, q.stride, 2*x + 1, 2*y + 1, q.depth);
      o1[(size_t)y*w1 + x] = v;
    }
    s1[ly][lx] = v;
  }
  __syncthreads();
  /* a sample of scale i + 1 inside its plane reads only samples of scale i inside theirs */
  {
    const int lx = tid%(kPyrTile/2);
    const int ly = tid/(kPyrTile/2);
    const int v = s1[2*ly][2*lx] + s1[2*ly][2*lx + 1] + s1[2*ly + 1][2*lx] + s1[2*ly + 1][2*lx + 1];
    const int x = bx/2 + lx;
    const int y = by/2 + ly;
    if (x < (q.w >> 2) && y < (q.h >> 2)) o2[(size_t)y*(q.w >> 2) + x] = v;
    s2[ly][lx] = v;
  }
  __syncthreads();
  if (tid < (kPyrTile/4)*(kPyrTile/4)) {
    const int lx = tid%(kPyrTile/4);
    const int ly = tid/(kPyrTile/4);
    const int v = s2[2*ly][2*lx] + s2[2*ly][2*lx + 1] + s2[2*ly + 1][2*lx] + s2[2*ly + 1][2*lx + 1];
    const int x = bx/4 + lx;
    const int y = by/4 + ly;
    if (x < (q.w >> 3) && y < (q.h >> 3)) o3[(size_t)y*(q.w >> 3) + x] = v;
    s3[ly][lx] = v;
  }
  __syncthreads();
  if (tid < (kPyrTile/8)*(kPyrTile/8)) {
    const int lx = tid%(kPyrTile/8);
    const int ly = tid/(kPyrTile/8);
    const int v = s3[2*ly][2*lx] + s3[2*ly][2*lx + 1] + s3[2*ly + 1][2*lx] + s3[2*ly + 1][2*lx + 1];
    const int x = bx/8 + lx;
    const int y = by/8 + ly;
    if (x < (q.w >> 4) && y < (q.h >> 4)) o4[(size_t)y*(q.w >> 4) + x] = v;
  }
}

/* the sum of the taps of position i of an axis of n samples that fall inside it */
__device__ __forceinline__ int clipped_weight(const int *tap, int i, int n) {
  int sum = 0;
  for (int k = max(0, kRadius - i); k < min(kTaps, kRadius + n - i); k++) sum += tap[k];
  return sum;
}

__global__ __launch_bounds__(kThreads) void k_msssim(MsBatch b, const int32_t *pyr, double *part, double *t_cs,
 double *t_ssim) {
  __shared__ int32_t sx[kSpan][kSpan];
  __shared__ int32_t sy[kSpan][kSpan];
  __shared__ long long hm[5][kRows][kTile];
  __shared__ int tap[kTaps];
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  const int e = find_entry(b.g.t.first, b.g.n*kScales, (int)blockIdx.x);
  const int pi = e/kScales;
  const int sc = e%kScales;
  const odhip_metrics_pair &q = b.p[pi];
  const int w = q.w >> sc;
  const int h = q.h >> sc;
  const int t = (int)blockIdx.x - b.g.t.first[e];
  const int ntx = (w + kTile - 1)/kTile;
  const int tx0 = (t%ntx)*kTile;
  const int ty0 = (t/ntx)*kTile;
  if (tid < kTaps) tap[tid] = kTapDev.t[tid];
  /* the staged columns and rows: the tile and its halo, clipped at the plane */
  const int c_lo = max(0, tx0 - kRadius);
  const int cw = min(w, tx0 + kTile + kRadius) - c_lo;
  const int r_lo = max(0, ty0 - kRadius);
  const int nr = min(h, ty0 + kTile + kRadius) - r_lo;
  if (sc == 0) {
    for (int i = tid; i < nr*cw; i += kThreads) {
      const int r = i/cw;
      const int c = i - r*cw;
      sx[r][c] = load_sample(q.src, q.src_fmt, q.src_stride, c_lo + c, r_lo + r, q.depth);
      sy[r][c] = load_sample(q.rec, q.rec_fmt, q.rec_stride, c_lo + c, r_lo + r, q.depth);
    }
  } else {
    const int32_t *ps = pyr + b.g.spyr[pi] + pyr_offset(q.w, q.h, sc);
    const int32_t *pr = pyr + b.g.rpyr[pi] + pyr_offset(q.w, q.h, sc);
    for (int i = tid; i < nr*cw; i += kThreads) {
      const int r = i/cw;
      const int c = i - r*cw;
      const size_t at = (size_t)(r_lo + r)*w + c_lo + c;
      sx[r][c] = ps[at];
      sy[r][c] = pr[at];
    }
  }
  const int ox = tid%kTile;
  const int oy = tid/kTile;
  const int x = tx0 + ox;
  long long acc[4][5];
#pragma unroll
  for (int j = 0; j < 4; j++) {
#pragma unroll
    for (int m = 0; m < 5; m++) acc[j][m] = 0;
  }
  for (int rb = 0; rb < nr; rb += kRows) {
    const int nrows = min(kRows, nr - rb);
    __syncthreads();                 /* the samples and taps are staged; the moments of the last group are read */
    if (oy < nrows) {
      long long mux = 0, muy = 0, x2 = 0, xy = 0, y2 = 0;
      if (x < w) {
        /* taps k with 0 <= x - 4 + k < w (dump_msssim.c:129-131) */
        const int k_min = max(0, kRadius - x);
        const int k_max = min(kTaps, kRadius + w - x);
        const int at = x - kRadius - c_lo;
#pragma unroll
        for (int k = 0; k < kTaps; k++) {
          if (k >= k_min && k < k_max) {
            const long long s = sx[rb + oy][at + k];
            const long long d = sy[rb + oy][at + k];
            const long long ws = kTapTable.t[k]*s;
            const long long wd = kTapTable.t[k]*d;
            mux += ws;
            muy += wd;
            x2 += ws*s;
            xy += ws*d;
            y2 += wd*d;
          }
        }
      }
      hm[0][oy][ox] = mux;
      hm[1][oy][ox] = muy;
      hm[2][oy][ox] = x2;
      hm[3][oy][ox] = xy;
      hm[4][oy][ox] = y2;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) {
      /* rows of this group with 0 <= row - y + 4 <= 8 (dump_msssim.c:152-153: rows outside the plane never come) */
      const int y = ty0 + oy + kRows*j;
      const int first = r_lo + rb;
      const int a = max(first, y - kRadius);
      const int z = min(first + nrows, y + kRadius + 1);
      for (int row = a; row < z; row++) {
        const long long win = tap[row - y + kRadius];
#pragma unroll
        for (int m = 0; m < 5; m++) acc[j][m] += win*hm[m][row - first][ox];
      }
    }
  }
  double sum = 0;
  if (x < w) {
    const int wx = clipped_weight(tap, x, w);
    const double smax = (double)(((1 << q.depth) - 1) << (2*sc));
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int y = ty0 + oy + kRows*j;
      if (y >= h) continue;
      const long long mw = (long long)wx*clipped_weight(tap, y, h);
      /* dump_msssim.c:175-184, operation by operation */
      const double wd = (double)mw;
      const double c1 = 0.01*0.01*smax*smax*wd*wd;
      const double c2 = 0.03*0.03*smax*smax*wd*wd;
      const double mx2 = (double)acc[j][0]*(double)acc[j][0];
      const double mxy = (double)acc[j][0]*(double)acc[j][1];
      const double my2 = (double)acc[j][1]*(double)acc[j][1];
      const double cs = (double)mw*(c2 + 2*((double)acc[j][3]*wd - mxy))
       /((double)acc[j][2]*wd - mx2 + (double)acc[j][4]*wd - my2 + c2);
      double term = cs;
      if (sc == kScales - 1 || t_ssim) {
        const double ssim = cs*(2*mxy + c1)/(mx2 + my2 + c1);
        if (t_ssim) t_ssim[(size_t)y*w + x] = ssim;
        if (sc == kScales - 1) term = ssim;
      }
      if (t_cs) t_cs[(size_t)y*w + x] = cs;
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

bool ms_pair_ok(const odhip_metrics_pair &q) {
  return pair_ok(q) && q.w >= kMinSize && q.h >= kMinSize;
}

struct MsTraits {
  static constexpr int kLevels = kScales;
  static size_t pyr_elems(int w, int h) { return pyr_offset(w, h, kScales); }
  static long pyr_blocks(int w, int h) {
    return (long)(((w >> 1) + kPyrTile - 1)/kPyrTile)*(((h >> 1) + kPyrTile - 1)/kPyrTile);
  }
  static long tiles(int w, int h, int sc) {
    return (long)(((w >> sc) + kTile - 1)/kTile)*(((h >> sc) + kTile - 1)/kTile);
  }
};

/* sum over positions 0..n-1 of the taps that fall inside */
int64_t axis_weight(int n) {
  int64_t sum = 0;
  for (int k = 0; k < kTaps; k++) {
    /* tap k reaches position i - 4 + k: inside for max(0, 4 - k) <= i < min(n, n + 4 - k) */
    const int lo = std::max(0, kRadius - k);
    const int hi = std::min(n, n + kRadius - k);
    if (hi > lo) sum += (int64_t)kTapTable.t[k]*(hi - lo);
  }
  return sum;
}

/* One launch group (metric_launch_build); only_scale >= 0: that scale alone, its term maps to t_cs / t_ssim. */
int ms_launch(MetricScratch *st, const odhip_metrics_pair *pairs, const int *idx, int m, int only_scale, double *d_sums,
 double *t_cs, double *t_ssim, hipStream_t s) {
  MetricLaunch L;
  const int rc = metric_launch_build<MsTraits>(&L, st, pairs, idx, m, only_scale, s);
  if (rc) return rc;
  MsBatch b;
  memset(&b, 0, sizeof(b));
  b.g = L.g;
  for (int i = 0; i < m; i++) b.p[i] = pairs[idx[i]];
  if (only_scale != 0) k_msssim_pyramid<<<(unsigned)L.blocks, kThreads, 0, s>>>(L.pb, L.nplanes, st->pyr.p);
  k_msssim<<<(unsigned)L.tiles, kThreads, 0, s>>>(b, st->pyr.p, st->part.p, t_cs, t_ssim);
  if (d_sums) metric_tile_sum(b.g.t, m, st->part.p, d_sums, s);
  return ODHIP_SUCCESS;
}

}  // namespace

/* gaussian_filter_init(1.5, 5) at weight 1024 (tools/dump_msssim.c:41-71), with the host libm; ODHIP_EIMPL if this
   libm's table is not the one the kernels were compiled with (taps[] is filled all the same) */
extern "C" int odhip_msssim_taps(uint32_t taps[9]) {
  if (!taps) return ODHIP_EINVAL;
  const double sigma = 1.5;
  const int max_len = 5;
  const double scale = 1/(sqrt(2*M_PI)*sigma);
  const double nhisigma2 = -0.5/(sigma*sigma);
  const double s = sqrt(0.5*M_PI)*sigma*(1.0/1024);
  const double len = s >= 1 ? 0 : floor(sigma*sqrt(-2*log(s)));
  const int n = len >= max_len ? max_len - 1 : (int)len;
  if (n != kRadius) return ODHIP_EIMPL;
  uint32_t sum = 0;
  for (int ci = n; ci > 0; ci--) {
    taps[n - ci] = taps[n + ci] = (uint32_t)(1024*scale*exp(nhisigma2*ci*ci) + 0.5);
    sum += taps[n - ci];
  }
  taps[n] = 1024 - (sum << 1);
  for (int k = 0; k < kTaps; k++) {
    if (taps[k] != (uint32_t)kTapTable.t[k]) return ODHIP_EIMPL;
  }
  return ODHIP_SUCCESS;
}

extern "C" int odhip_msssim_weights(int w, int h, int64_t weight[5]) {
  if (w < kMinSize || h < kMinSize || w > 65535 || h > 65535 || !weight) return ODHIP_EINVAL;
  for (int sc = 0; sc < kScales; sc++) weight[sc] = axis_weight(w >> sc)*axis_weight(h >> sc);
  return ODHIP_SUCCESS;
}

/* calc_msssim's product (tools/dump_msssim.c:268-269) with the host libm's pow: a negative value gives NAN there too */
extern "C" int odhip_msssim_score(const double sums[5], const int64_t weight[5], double *score) {
  static const double kExponent[kScales] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  if (!sums || !weight || !score) return ODHIP_EINVAL;
  for (int sc = 0; sc < kScales; sc++) {
    if (weight[sc] <= 0) return ODHIP_EINVAL;
  }
  double v[kScales];
  for (int sc = 0; sc < kScales; sc++) v[sc] = sums[sc]/(double)weight[sc];
  *score = pow(v[0], kExponent[0])*pow(v[1], kExponent[1])*pow(v[2], kExponent[2])*pow(v[3], kExponent[3])
   *pow(v[4], kExponent[4]);
  return ODHIP_SUCCESS;
}

extern "C" int odhip_msssim_prepare(int w, int h, int pairs) {
  if (w < kMinSize || h < kMinSize || w > 65535 || h > 65535 || pairs < 1) return ODHIP_EINVAL;
  ODHIP_CTX_OR_RETURN(ctx);
  return metric_prepare<MsTraits>(odhip_ctx_state<MetricScratch>(ctx, ODHIP_SLOT_MSSSIM), w, h, pairs);
}

extern "C" int odhip_msssim_planes(const odhip_metrics_pair *pairs, int n, double *d_sums, int64_t *weights,
 odhip_stream stream) {
  if (n < 0 || !pairs || !d_sums) return ODHIP_EINVAL;
  for (int i = 0; i < n; i++) {
    if (!ms_pair_ok(pairs[i])) return ODHIP_EINVAL;
  }
  if (n == 0) return ODHIP_SUCCESS;
  ODHIP_CTX_OR_RETURN(ctx);
  MetricScratch *st = odhip_ctx_state<MetricScratch>(ctx, ODHIP_SLOT_MSSSIM);
  int rc = metric_planes<MsTraits>(pairs, n, [&](const int *idx, int m) {
    return ms_launch(st, pairs, idx, m, -1, d_sums, nullptr, nullptr, (hipStream_t)stream);
  });
  if (rc) return rc;
  if (weights) {
    for (int i = 0; i < n; i++) {
      rc = odhip_msssim_weights(pairs[i].w, pairs[i].h, weights + (size_t)i*kScales);
      if (rc) return rc;
    }
  }
  return odhip_check_launch();
}

extern "C" int odhip_msssim_terms(const odhip_metrics_pair *pair, int scale, double *d_cs, double *d_ssim,
 odhip_stream stream) {
  if (!pair || !d_cs || !d_ssim || scale < 0 || scale >= kScales || !ms_pair_ok(*pair)) return ODHIP_EINVAL;
  ODHIP_CTX_OR_RETURN(ctx);
  const int idx = 0;
  const int rc = ms_launch(odhip_ctx_state<MetricScratch>(ctx, ODHIP_SLOT_MSSSIM), pair, &idx, 1, scale, nullptr, d_cs,
   d_ssim, (hipStream_t)stream);
  return rc ? rc : odhip_check_launch();
}
