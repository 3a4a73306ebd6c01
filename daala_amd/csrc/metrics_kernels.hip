/* metrics_kernels.hip - the distortion side of a rate-distortion curve: PSNR and PSNR-HVS-M of
   source / reconstruction plane pairs on the device (what the reference's tools/dump_psnr.c and
   tools/dump_psnrhvs.c compute from decoded Y4M files).

   Both metrics run over the PICTURE region of a plane at the source depth D (8, 10, 12).  A sample
   is read as uint8 (D = 8), uint16 (depth D) or int16 at 12 bits - the pipe's full-precision planes -
   brought down to D by the reference's output conversion OD_CLAMPI(0, (s + (1 << sh >> 1)) >> sh,
   (1 << D) - 1), sh = 12 - D (od_img_plane_copy, src/state.c:158-182).  A padded source plane holds
   src << sh, which the same conversion gives back exactly.

   k_metrics       grid (kChunks, pairs): chunk k of a pair takes a fixed share of the pixel rows (SSE:
                   int64, exact in any order) and of the window rows of PSNR-HVS-M.  One lane per 8x8
                   window at step 7 (calc_psnrhvs, dump_psnrhvs.c:62-165): means and variances in single
                   precision in the tool's order, od_bin_fdct8x8 of both windows through the 8-point
                   lifting network (od_lift.cuh, bit-exact with src/dct.c), the masking terms (sqrt of
                   the float product in double, as C evaluates it) and the 64 float terms (err*csf)^2.
                   The tool adds every term of a plane into one running float, which no parallel order
                   reproduces; here a lane adds its windows' float terms in double, the workgroup
                   reduces its lanes in a fixed tree and a chunk leaves one partial, so a result repeats
                   from run to run.
   k_metrics_sum   one lane per pair: the chunk partials in chunk order -> sse[pair], hvs[pair].
   k_hvs_windows   test surface: one lane per window, its 64 terms summed in float in (i, j) order.

   The host divides by the pixel count (PSNR) or by 64 x windows and samplemax^2 (PSNR-HVS-M).

   SSIM (calc_ssim, tools/dump_ssim.c:79-189): an integer Gaussian of weight 256 along the rows, then down
   the columns, over the moments mux, muy, x2, xy, y2 and the weight w; taps outside the plane are dropped
   (the halo is clipped, never clamped or mirrored: the truncation and the weight are the metric).  The tap
   tables come from the HOST libm (odhip_ssim_taps, as gaussian_filter_init builds them) and are kept per
   context on the device, one entry per (w, h, par).
   k_ssim          one workgroup per 32x32 output tile of a pair (a flat grid over the tiles of the batch).
                   The tile's rows and kSsimMaxRadius rows above and below go through LDS kSsimRows at a
                   time: both planes' samples with the column halo (uint16), then their horizontal moments
                   (uint32: below 2^32 at 12 bits); a lane owns one column and four rows of the tile and
                   adds tap x moment into int64 registers (below 2^41).  The weight is separable (row sum x
                   column sum).  The per-sample term is the tool's double expression, one IEEE operation
                   per C operation in its association (-ffp-contract=off); the lane adds its four terms in
                   row order, the workgroup reduces in a fixed tree and leaves one partial per tile.
   The launch groups (the call's order, no source plane shared) and k_metric_tile_sum, which adds a pair's partials
   in a fixed order -> sum[pair], are od_metric_launch.cuh's.
   The largest radius is kSsimMaxRadius = ODHIP_SSIM_MAX_RADIUS = 64 (coded heights up to 5000 and more):
   the staged row is 32 + 2 x 64 samples wide.  LDS: 10 KiB samples + 10 KiB moments + 3 KiB. */
#include <math.h>
#include <string.h>
#include <vector>
#include "../../include/daala_hip.h"
#include "od_ctx.cuh"
#include "od_lift.cuh"
#include "od_metric_launch.cuh"
#include "od_sample.cuh"
#include "gen/od_csf_tables.h"

namespace {

constexpr int kChunks = 64;          /* partials per pair; kThreads and kBatch are od_metric_launch.cuh's */

struct MetricBatch {
  odhip_metrics_pair p[kBatch];
  int flags;
};

/* (float)((csf*k)*(csf*k)) in double, dump_psnrhvs.c:90 - evaluated by the compiler */
struct MaskTables {
  float m[3][8][8];
};
constexpr MaskTables make_masks() {
  MaskTables t{};
  for (int c = 0; c < 3; c++) {
    for (int i = 0; i < 8; i++) {
      for (int j = 0; j < 8; j++) {
        const double v = (double)OD_CSF[c][i][j]*0.3885746225901003;
        t.m[c][i][j] = (float)(v*v);
      }
    }
  }
  return t;
}
__constant__ MaskTables kMask = make_masks();
__constant__ float kCsf[3][8][8] = {
#define OD_CSF_ROW(c, i) {OD_CSF[c][i][0], OD_CSF[c][i][1], OD_CSF[c][i][2], OD_CSF[c][i][3], OD_CSF[c][i][4], \
  OD_CSF[c][i][5], OD_CSF[c][i][6], OD_CSF[c][i][7]}
#define OD_CSF_TAB(c) {OD_CSF_ROW(c, 0), OD_CSF_ROW(c, 1), OD_CSF_ROW(c, 2), OD_CSF_ROW(c, 3), OD_CSF_ROW(c, 4), \
  OD_CSF_ROW(c, 5), OD_CSF_ROW(c, 6), OD_CSF_ROW(c, 7)}
  OD_CSF_TAB(0), OD_CSF_TAB(1), OD_CSF_TAB(2)
#undef OD_CSF_TAB
#undef OD_CSF_ROW
};

/* od_bin_fdct8x8 (src/dct.c): od_bin_fdct8 down every column, then along every row of that result;
   x[i][j] -> x[u][v], u the vertical frequency */
__device__ __forceinline__ void fdct8x8(OdMul32 (&x)[8][8]) {
  OdMul32 z[8][8];
#pragma unroll
  for (int c = 0; c < 8; c++) {
    OdMul32 in[8];
    OdMul32 out[8];
#pragma unroll
    for (int k = 0; k < 8; k++) in[k] = x[k][c];
    od_fdct8_lift(out, in);
#pragma unroll
    for (int k = 0; k < 8; k++) z[c][k] = out[k];
  }
#pragma unroll
  for (int r = 0; r < 8; r++) {
    OdMul32 in[8];
    OdMul32 out[8];
#pragma unroll
    for (int k = 0; k < 8; k++) in[k] = z[k][r];
    od_fdct8_lift(out, in);
#pragma unroll
    for (int k = 0; k < 8; k++) x[r][k] = out[k];
  }
}

/* The 8x8 window of calc_psnrhvs at (x, y): term(t) receives its 64 float terms in (i, j) order.  Every
   operation is the tool's, in its order and precision (-ffp-contract=off: no fused multiply-adds). */
template <class Term>
__device__ __forceinline__ void hvs_window(const odhip_metrics_pair &q, int x, int y, Term term) {
  const float(&csf)[8][8] = kCsf[q.csf];
  const float(&mask)[8][8] = kMask.m[q.csf];
  OdMul32 s[8][8];
  OdMul32 d[8][8];
  float s_means[4] = {0, 0, 0, 0};
  float d_means[4] = {0, 0, 0, 0};
  float s_vars[4] = {0, 0, 0, 0};
  float d_vars[4] = {0, 0, 0, 0};
  float s_gmean = 0;
  float d_gmean = 0;
  float s_gvar = 0;
  float d_gvar = 0;
  float s_mask = 0;
  float d_mask = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int sub = ((i & 12) >> 2) + ((j & 12) >> 1);
      s[i][j] = OdMul32(load_sample(q.src, q.src_fmt, q.src_stride, x + j, y + i, q.depth));
      d[i][j] = OdMul32(load_sample(q.rec, q.rec_fmt, q.rec_stride, x + j, y + i, q.depth));
      s_gmean += (float)s[i][j].v;
      d_gmean += (float)d[i][j].v;
      s_means[sub] += (float)s[i][j].v;
      d_means[sub] += (float)d[i][j].v;
    }
  }
  s_gmean /= 64.f;
  d_gmean /= 64.f;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    s_means[i] /= 16.f;
    d_means[i] /= 16.f;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int sub = ((i & 12) >> 2) + ((j & 12) >> 1);
      const float sv = (float)s[i][j].v;
      const float dv = (float)d[i][j].v;
      s_gvar += (sv - s_gmean)*(sv - s_gmean);
      d_gvar += (dv - d_gmean)*(dv - d_gmean);
      s_vars[sub] += (sv - s_means[sub])*(sv - s_means[sub]);
      d_vars[sub] += (dv - d_means[sub])*(dv - d_means[sub]);
    }
  }
  constexpr float k63 = 1/63.f*64;
  constexpr float k15 = 1/15.f*16;
  s_gvar *= k63;
  d_gvar *= k63;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    s_vars[i] *= k15;
    d_vars[i] *= k15;
  }
  if (s_gvar > 0) s_gvar = (s_vars[0] + s_vars[1] + s_vars[2] + s_vars[3])/s_gvar;
  if (d_gvar > 0) d_gvar = (d_vars[0] + d_vars[1] + d_vars[2] + d_vars[3])/d_gvar;
  fdct8x8(s);
  fdct8x8(d);
#pragma unroll
  for (int i = 0; i < 8; i++) {
#pragma unroll
    for (int j = (i == 0); j < 8; j++) s_mask += (float)(s[i][j].v*s[i][j].v)*mask[i][j];
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
#pragma unroll
    for (int j = (i == 0); j < 8; j++) d_mask += (float)(d[i][j].v*d[i][j].v)*mask[i][j];
  }
  s_mask = (float)(__dsqrt_rn((double)(s_mask*s_gvar))/32.);
  d_mask = (float)(__dsqrt_rn((double)(d_mask*d_gvar))/32.);
  if (d_mask > s_mask) s_mask = d_mask;
#pragma unroll
  for (int i = 0; i < 8; i++) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float err = (float)abs(s[i][j].v - d[i][j].v);
      if (i != 0 || j != 0) {
        const float m = s_mask/mask[i][j];
        err = err < m ? 0.f : err - m;
      }
      term((err*csf[i][j])*(err*csf[i][j]));
    }
  }
}

/* rows [a, b) of n: share k of kChunks */
__device__ __forceinline__ void chunk_rows(int n, int k, int &a, int &b) {
  a = (int)((long)n*k/kChunks);
  b = (int)((long)n*(k + 1)/kChunks);
}

__device__ __forceinline__ int window_span(int n) {
  return n > 7 ? (n - 7 + 6)/7 : 0;
}

__global__ __launch_bounds__(kThreads) void k_metrics(MetricBatch b, long long *part_sse, double *part_hvs) {
  __shared__ long long ls[kThreads];
  __shared__ double lh[kThreads];
  const odhip_metrics_pair &q = b.p[blockIdx.y];
  const int k = blockIdx.x;
  const int tid = threadIdx.x;
  long long sse = 0;
  double hvs = 0;
  if (b.flags & ODHIP_METRIC_SSE) {
    int y0, y1;
    chunk_rows(q.h, k, y0, y1);
    for (int y = y0; y < y1; y++) {
      for (int x = tid; x < q.w; x += kThreads) {
        const int e = load_sample(q.src, q.src_fmt, q.src_stride, x, y, q.depth)
         - load_sample(q.rec, q.rec_fmt, q.rec_stride, x, y, q.depth);
        sse += (long long)(e*e);
      }
    }
  }
  if (b.flags & ODHIP_METRIC_PSNRHVS) {
    /* windows at (7 wx, 7 wy) with 7 wx < w - 7, 7 wy < h - 7 */
    const int nwx = window_span(q.w);
    int r0, r1;
    chunk_rows(window_span(q.h), k, r0, r1);
    const int n = (r1 - r0)*nwx;
    for (int i = tid; i < n; i += kThreads) {
      const int wy = r0 + i/nwx;
      const int wx = i%nwx;
      hvs_window(q, 7*wx, 7*wy, [&](float t) { hvs += (double)t; });
    }
  }
  ls[tid] = sse;
  lh[tid] = hvs;
  __syncthreads();
  for (int s = kThreads/2; s > 0; s >>= 1) {
    if (tid < s) {
      ls[tid] += ls[tid + s];
      lh[tid] += lh[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    part_sse[blockIdx.y*kChunks + k] = ls[0];
    part_hvs[blockIdx.y*kChunks + k] = lh[0];
  }
}

__global__ __launch_bounds__(64) void k_metrics_sum(int n, int flags, const long long *part_sse,
 const double *part_hvs, int64_t *sse, double *hvs) {
  const int i = blockIdx.x*64 + threadIdx.x;
  if (i >= n) return;
  long long a = 0;
  double h = 0;
  for (int k = 0; k < kChunks; k++) {
    a += part_sse[i*kChunks + k];
    h += part_hvs[i*kChunks + k];
  }
  if (flags & ODHIP_METRIC_SSE) sse[i] = a;
  if (flags & ODHIP_METRIC_PSNRHVS) hvs[i] = h;
}

__global__ __launch_bounds__(kThreads) void k_hvs_windows(odhip_metrics_pair q, int nwx, int nwy, float *out) {
  const int i = blockIdx.x*kThreads + threadIdx.x;
  if (i >= nwx*nwy) return;
  float ret = 0;
  hvs_window(q, 7*(i%nwx), 7*(i/nwx), [&](float t) { ret += t; });
  out[i] = ret;
}

/* ---- SSIM ---- */
constexpr int kSsimMaxRadius = ODHIP_SSIM_MAX_RADIUS;
constexpr int kSsimTapLen = 2*kSsimMaxRadius + 1;
constexpr int kSsimTile = kTile;                      /* a lane owns 1 column x 4 rows of the output tile */
constexpr int kSsimRows = 16;                         /* rows in LDS at a time */
constexpr int kSsimSpan = kSsimTile + 2*kSsimMaxRadius;
constexpr int kSsimTapSlots = 64;                     /* tap table entries per context */
static_assert(kThreads == kSsimTile*8, "k_ssim: 8 lanes down a tile column");

struct SsimBatch {
  odhip_metrics_pair p[kBatch];
  MetricTiles t;                                      /* one column: first[i] is the first tile of pair i */
  int entry[kBatch];                                  /* its tap table entry */
  short vr[kBatch];
  short hr[kBatch];
};

__global__ __launch_bounds__(kThreads) void k_ssim(SsimBatch b, const uint32_t *taps, double *part, double *terms) {
  __shared__ uint16_t sx[kSsimRows][kSsimSpan];
  __shared__ uint16_t sy[kSsimRows][kSsimSpan];
  __shared__ uint32_t hm[5][kSsimRows][kSsimTile];
  __shared__ uint32_t tv[kSsimTapLen];
  __shared__ uint32_t th[kSsimTapLen];
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  int pi = 0;
  while ((int)blockIdx.x >= b.t.first[pi + 1]) pi++;
  const odhip_metrics_pair &q = b.p[pi];
  const int vr = b.vr[pi];
  const int hr = b.hr[pi];
  const int w = q.w;
  const int h = q.h;
  const int t = (int)blockIdx.x - b.t.first[pi];
  const int ntx = (w + kSsimTile - 1)/kSsimTile;
  const int tx0 = (t%ntx)*kSsimTile;
  const int ty0 = (t/ntx)*kSsimTile;
  const uint32_t *tab = taps + (size_t)b.entry[pi]*2*kSsimTapLen;
  for (int i = tid; i < 2*vr + 1; i += kThreads) tv[i] = tab[i];
  for (int i = tid; i < 2*hr + 1; i += kThreads) th[i] = tab[kSsimTapLen + i];
  /* the staged columns and rows: the tile and its halo, clipped at the plane */
  const int c_lo = max(0, tx0 - hr);
  const int cw = min(w, tx0 + kSsimTile + hr) - c_lo;
  const int r_lo = max(0, ty0 - vr);
  const int r_hi = min(h, ty0 + kSsimTile + vr);
  const int ox = tid%kSsimTile;
  const int oy = tid/kSsimTile;
  const int x = tx0 + ox;
  long long acc[4][5];
#pragma unroll
  for (int j = 0; j < 4; j++) {
#pragma unroll
    for (int m = 0; m < 5; m++) acc[j][m] = 0;
  }
  for (int rb = r_lo; rb < r_hi; rb += kSsimRows) {
    const int nrows = min(kSsimRows, r_hi - rb);
    __syncthreads();
    for (int i = tid; i < nrows*cw; i += kThreads) {
      const int r = i/cw;
      const int c = i - r*cw;
      sx[r][c] = (uint16_t)load_sample(q.src, q.src_fmt, q.src_stride, c_lo + c, rb + r, q.depth);
      sy[r][c] = (uint16_t)load_sample(q.rec, q.rec_fmt, q.rec_stride, c_lo + c, rb + r, q.depth);
    }
    __syncthreads();
    for (int i = tid; i < nrows*kSsimTile; i += kThreads) {
      const int r = i/kSsimTile;
      const int xi = i%kSsimTile;
      const int xx = tx0 + xi;
      uint32_t mux = 0, muy = 0, x2 = 0, xy = 0, y2 = 0;
      if (xx < w) {
        /* taps k with 0 <= xx - hr + k < w (dump_ssim.c:120-122) */
        const int k_min = max(0, hr - xx);
        const int k_max = min(2*hr + 1, hr + w - xx);
        const int at = xx - hr - c_lo;
        for (int k = k_min; k < k_max; k++) {
          const uint32_t win = th[k];
          const uint32_t s = sx[r][at + k];
          const uint32_t d = sy[r][at + k];
          mux += win*s;
          muy += win*d;
          x2 += win*s*s;
          xy += win*s*d;
          y2 += win*d*d;
        }
      }
      hm[0][r][xi] = mux;
      hm[1][r][xi] = muy;
      hm[2][r][xi] = x2;
      hm[3][r][xi] = xy;
      hm[4][r][xi] = y2;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) {
      /* rows of this batch with 0 <= row - y + vr <= 2 vr (dump_ssim.c:150-151: rows outside the plane never come) */
      const int y = ty0 + oy + 8*j;
      const int a = max(rb, y - vr);
      const int e = min(rb + nrows, y + vr + 1);
      for (int row = a; row < e; row++) {
        const long long win = tv[row - y + vr];
#pragma unroll
        for (int m = 0; m < 5; m++) acc[j][m] += win*(long long)hm[m][row - rb][ox];
      }
    }
  }
  double sum = 0;
  if (x < w) {
    long long wx = 0;
    for (int k = max(0, hr - x); k < min(2*hr + 1, hr + w - x); k++) wx += th[k];
    const double smax2 = (double)(((1 << q.depth) - 1)*((1 << q.depth) - 1));
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int y = ty0 + oy + 8*j;
      if (y >= h) continue;
      long long wy = 0;
      for (int k = max(0, vr - y); k < min(2*vr + 1, vr + h - y); k++) wy += tv[k];
      const long long mw = wx*wy;
      /* dump_ssim.c:172-179, operation by operation */
      const double wd = (double)mw;
      const double c1 = smax2*(0.01*0.01)*wd*wd;
      const double c2 = smax2*(0.03*0.03)*wd*wd;
      const double mx2 = (double)acc[j][0]*(double)acc[j][0];
      const double mxy = (double)acc[j][0]*(double)acc[j][1];
      const double my2 = (double)acc[j][1]*(double)acc[j][1];
      const double term = (double)mw*(2*mxy + c1)*(c2 + 2*((double)acc[j][3]*wd - mxy))
       /((mx2 + my2 + c1)*((double)acc[j][2]*wd - mx2 + (double)acc[j][4]*wd - my2 + c2));
      if (terms) terms[(long)y*w + x] = term;
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

/* the chunk partials of one batch, per context (one call sequence in flight per context) */
struct SsimTapKey {
  int w, h;
  double par;
  int vr, hr;                  /* radii of the vertical and the horizontal table */
};
struct MetricsState {
  DeviceBuf<long long> part_sse;
  DeviceBuf<double> part_hvs;
  /* SSIM: tile partials of one launch, and the tap tables seen so far (entry e: kSsimTapLen vertical taps, then
     kSsimTapLen horizontal ones) */
  DeviceBuf<double> part_ssim;
  DeviceBuf<uint32_t> taps;
  std::vector<SsimTapKey> tap_keys;
  std::vector<uint32_t> tap_host;
};

}  // namespace

extern "C" long odhip_psnrhvs_window_count(int w, int h, int *nwx, int *nwy) {
  const int ax = w > 7 ? (w - 7 + 6)/7 : 0;
  const int ay = h > 7 ? (h - 7 + 6)/7 : 0;
  if (nwx) *nwx = ax;
  if (nwy) *nwy = ay;
  return (long)ax*ay;
}

extern "C" int odhip_metrics_prepare(void) {
  ODHIP_CTX_OR_RETURN(ctx);
  MetricsState *st = odhip_ctx_state<MetricsState>(ctx, ODHIP_SLOT_METRICS);
  const int rc = st->part_sse.reserve((size_t)kBatch*kChunks);
  return rc ? rc : st->part_hvs.reserve((size_t)kBatch*kChunks);
}

extern "C" int odhip_metrics_planes(const odhip_metrics_pair *pairs, int n, int flags, int64_t *d_sse,
 double *d_hvs, long *npixels, long *nwindows, odhip_stream stream) {
  if (n < 0 || (n > 0 && !pairs) || flags == 0 || (flags & ~(ODHIP_METRIC_SSE | ODHIP_METRIC_PSNRHVS))) {
    return ODHIP_EINVAL;
  }
  if (((flags & ODHIP_METRIC_SSE) && !d_sse) || ((flags & ODHIP_METRIC_PSNRHVS) && !d_hvs)) return ODHIP_EINVAL;
  for (int i = 0; i < n; i++) {
    if (!pair_ok(pairs[i])) return ODHIP_EINVAL;
  }
  for (int i = 0; i < n; i++) {
    if (npixels) npixels[i] = (long)pairs[i].w*pairs[i].h;
    if (nwindows) nwindows[i] = odhip_psnrhvs_window_count(pairs[i].w, pairs[i].h, nullptr, nullptr);
  }
  if (n == 0) return ODHIP_SUCCESS;
  const int rc = odhip_metrics_prepare();
  if (rc) return rc;
  MetricsState *st = odhip_ctx_state<MetricsState>(odhip_ctx_current(), ODHIP_SLOT_METRICS);
  hipStream_t s = (hipStream_t)stream;
  for (int first = 0; first < n; first += kBatch) {
    const int m = n - first < kBatch ? n - first : kBatch;
    MetricBatch b;
    for (int i = 0; i < m; i++) b.p[i] = pairs[first + i];
    b.flags = flags;
    k_metrics<<<dim3(kChunks, (unsigned)m), kThreads, 0, s>>>(b, st->part_sse.p, st->part_hvs.p);
    k_metrics_sum<<<1, 64, 0, s>>>(m, flags, st->part_sse.p, st->part_hvs.p, d_sse ? d_sse + first : nullptr,
     d_hvs ? d_hvs + first : nullptr);
  }
  return odhip_check_launch();
}

extern "C" int odhip_psnrhvs_windows(const odhip_metrics_pair *pair, float *d_out, odhip_stream stream) {
  if (!pair || !d_out || !pair_ok(*pair)) return ODHIP_EINVAL;
  int nwx = 0;
  int nwy = 0;
  const long nw = odhip_psnrhvs_window_count(pair->w, pair->h, &nwx, &nwy);
  if (nw == 0) return ODHIP_SUCCESS;
  if (nw > 0x7fffffffL - kThreads) return ODHIP_EINVAL;
  k_hvs_windows<<<(unsigned)((nw + kThreads - 1)/kThreads), kThreads, 0, (hipStream_t)stream>>>(*pair, nwx, nwy,
   d_out);
  return odhip_check_launch();
}

/* ---- SSIM: host side ---- */
namespace {

/* The tap table of a Gaussian of weight 256 (gaussian_filter_init, tools/dump_ssim.c:33-63), with the host libm. */
std::vector<uint32_t> ssim_taps(double sigma, int max_len) {
  const double scale = 1/(sqrt(2*M_PI)*sigma);
  const double nhisigma2 = -0.5/(sigma*sigma);
  const double s = sqrt(0.5*M_PI)*sigma*(1.0/256);
  const double len = s >= 1 ? 0 : floor(sigma*sqrt(-2*log(s)));
  const int n = len >= max_len ? max_len - 1 : (int)len;
  std::vector<uint32_t> t((size_t)2*n + 1);
  uint32_t sum = 0;
  for (int ci = n; ci > 0; ci--) {
    t[n - ci] = t[n + ci] = (uint32_t)(256*scale*exp(nhisigma2*ci*ci) + 0.5);
    sum += t[n - ci];
  }
  t[n] = 256 - (sum << 1);
  return t;
}

bool par_ok(double par) {
  return par > 0 && par <= 1e6 && par >= 1e-6;
}

void ssim_plane_taps(int w, int h, double par, std::vector<uint32_t> &vt, std::vector<uint32_t> &ht) {
  const int max_len = w < h ? w : h;
  vt = ssim_taps(h*(1.5/256), max_len);
  ht = ssim_taps(h*(1.5/256)/par, max_len);
}

/* sum over positions 0..n-1 of the taps that fall inside */
int64_t ssim_axis_weight(const std::vector<uint32_t> &t, int n) {
  const int r = (int)(t.size()/2);
  int64_t sum = 0;
  for (int k = 0; k < (int)t.size(); k++) {
    /* tap k reaches position i - r + k: inside for max(0, r - k) <= i < min(n, n + r - k) */
    const int lo = r - k > 0 ? r - k : 0;
    const int hi = n + r - k < n ? n + r - k : n;
    if (hi > lo) sum += (int64_t)t[k]*(hi - lo);
  }
  return sum;
}

/* The device entry of the tables of (w, h, par), uploaded on `s` at first sight.  ODHIP_EIMPL: a radius above
   kSsimMaxRadius, or a table the uint32 moments cannot carry (a centre tap that went negative). */
int ssim_find(const MetricsState *st, int w, int h, double par) {
  for (size_t i = 0; i < st->tap_keys.size(); i++) {
    const SsimTapKey &k = st->tap_keys[i];
    if (k.w == w && k.h == h && k.par == par) return (int)i;
  }
  return -1;
}

/* ODHIP_EIMPL for a plane whose radius the tiling does not take; nothing is launched or uploaded */
int ssim_radius_check(const MetricsState *st, int w, int h, double par) {
  if (ssim_find(st, w, h, par) >= 0) return ODHIP_SUCCESS;
  std::vector<uint32_t> vt, ht;
  ssim_plane_taps(w, h, par, vt, ht);
  return vt.size() > (size_t)kSsimTapLen || ht.size() > (size_t)kSsimTapLen ? ODHIP_EIMPL : ODHIP_SUCCESS;
}

int ssim_entry(MetricsState *st, int w, int h, double par, hipStream_t s, int *entry, int *vr, int *hr) {
  const int at = ssim_find(st, w, h, par);
  if (at >= 0) {
    *entry = at;
    *vr = st->tap_keys[at].vr;
    *hr = st->tap_keys[at].hr;
    return ODHIP_SUCCESS;
  }
  std::vector<uint32_t> vt, ht;
  ssim_plane_taps(w, h, par, vt, ht);
  if (vt.size() > (size_t)kSsimTapLen || ht.size() > (size_t)kSsimTapLen) return ODHIP_EIMPL;
  for (uint32_t v : vt) if (v > 256) return ODHIP_EIMPL;
  for (uint32_t v : ht) if (v > 256) return ODHIP_EIMPL;
  if (st->tap_keys.size() == (size_t)kSsimTapSlots) {
    /* every entry is taken: launches in flight read them - wait, then start over */
    ODHIP_TRY(hipDeviceSynchronize());
    st->tap_keys.clear();
  }
  const size_t e = st->tap_keys.size();
  uint32_t *host = st->tap_host.data() + e*2*kSsimTapLen;
  memset(host, 0, sizeof(uint32_t)*2*kSsimTapLen);
  memcpy(host, vt.data(), sizeof(uint32_t)*vt.size());
  memcpy(host + kSsimTapLen, ht.data(), sizeof(uint32_t)*ht.size());
  ODHIP_TRY(hipMemcpyAsync(st->taps.p + e*2*kSsimTapLen, host, sizeof(uint32_t)*2*kSsimTapLen, hipMemcpyHostToDevice, s));
  st->tap_keys.push_back(SsimTapKey{w, h, par, (int)(vt.size()/2), (int)(ht.size()/2)});
  *entry = (int)e;
  *vr = (int)(vt.size()/2);
  *hr = (int)(ht.size()/2);
  return ODHIP_SUCCESS;
}

long ssim_tiles(int w, int h) {
  return (long)((w + kSsimTile - 1)/kSsimTile)*((h + kSsimTile - 1)/kSsimTile);
}

int ssim_scratch(MetricsState *st, long tiles) {
  if (!st->taps.p) {
    const int rc = st->taps.alloc((size_t)2*kSsimTapLen*kSsimTapSlots);
    if (rc) return rc;
    st->tap_host.assign((size_t)2*kSsimTapLen*kSsimTapSlots, 0);
  }
  return st->part_ssim.reserve((size_t)tiles);     /* frees first: hipFree syncs the device */
}

/* One launch group: the pairs pairs[idx[0 .. m)], m <= kBatch, their radii checked; their sums go to d_sum[idx[i]] */
int ssim_launch(MetricsState *st, const odhip_metrics_pair *pairs, const int *idx, int m, double par, double *d_sum,
 double *d_terms, hipStream_t s) {
  SsimBatch b;
  memset(&b, 0, sizeof(b));
  int tiles = 0;
  for (int i = 0; i < m; i++) {
    b.p[i] = pairs[idx[i]];
    b.t.first[i] = tiles;
    b.t.out[i] = idx[i];
    tiles += (int)ssim_tiles(b.p[i].w, b.p[i].h);
  }
  for (int i = m; i <= kBatch; i++) b.t.first[i] = tiles;
  b.t.columns = 1;
  int rc = ssim_scratch(st, tiles);
  if (rc) return rc;
  for (int i = 0; i < m; i++) {
    /* an entry found here stays valid for this launch: a full table is emptied only behind a device sync, and
       the entries of one launch are at most kBatch <= kSsimTapSlots */
    const int before = (int)st->tap_keys.size();
    int vr = 0, hr = 0;
    rc = ssim_entry(st, b.p[i].w, b.p[i].h, par, s, &b.entry[i], &vr, &hr);
    if (rc) return rc;
    b.vr[i] = (short)vr;
    b.hr[i] = (short)hr;
    if ((int)st->tap_keys.size() < before) i = -1;                  /* the table started over: look all up again */
  }
  k_ssim<<<(unsigned)tiles, kThreads, 0, s>>>(b, st->taps.p, st->part_ssim.p, d_terms);
  if (d_sum) metric_tile_sum(b.t, m, st->part_ssim.p, d_sum, s);
  return ODHIP_SUCCESS;
}

}  // namespace

extern "C" int odhip_ssim_taps(double sigma, int max_len, uint32_t *taps, int cap) {
  if (!(sigma > 0) || sigma > 1e6 || max_len < 1 || !taps) return ODHIP_EINVAL;
  const std::vector<uint32_t> t = ssim_taps(sigma, max_len);
  if ((size_t)cap < t.size() || cap < 0) return ODHIP_EINVAL;
  memcpy(taps, t.data(), sizeof(uint32_t)*t.size());
  return (int)t.size();
}

extern "C" int odhip_ssim_weight(int w, int h, double par, int64_t *weight) {
  if (w < 1 || h < 1 || w > 65535 || h > 65535 || !par_ok(par) || !weight) return ODHIP_EINVAL;
  std::vector<uint32_t> vt, ht;
  ssim_plane_taps(w, h, par, vt, ht);
  *weight = ssim_axis_weight(ht, w)*ssim_axis_weight(vt, h);
  return ODHIP_SUCCESS;
}

extern "C" int odhip_ssim_prepare(long tiles) {
  ODHIP_CTX_OR_RETURN(ctx);
  if (tiles < 1) return ODHIP_EINVAL;
  return ssim_scratch(odhip_ctx_state<MetricsState>(ctx, ODHIP_SLOT_METRICS), tiles);
}

extern "C" long odhip_ssim_tile_count(int w, int h) {
  return w > 0 && h > 0 ? ssim_tiles(w, h) : 0;
}

extern "C" int odhip_ssim_planes(const odhip_metrics_pair *pairs, int n, double par, double *d_sum, int64_t *weights,
 odhip_stream stream) {
  if (n < 0 || (n > 0 && (!pairs || !d_sum)) || !par_ok(par)) return ODHIP_EINVAL;
  for (int i = 0; i < n; i++) {
    if (!pair_ok(pairs[i])) return ODHIP_EINVAL;
  }
  if (n == 0) return ODHIP_SUCCESS;
  ODHIP_CTX_OR_RETURN(ctx);
  MetricsState *st = odhip_ctx_state<MetricsState>(ctx, ODHIP_SLOT_METRICS);
  hipStream_t s = (hipStream_t)stream;
  /* every table first: a radius above the tiling's refuses the call before any launch */
  for (int i = 0; i < n; i++) {
    const int rc = ssim_radius_check(st, pairs[i].w, pairs[i].h, par);
    if (rc) return rc;
  }
  /* no pyramid, so no plane to share: groups in the call's order */
  const MetricGroups g = metric_groups(pairs, n, [](const odhip_metrics_pair &q) { return ssim_tiles(q.w, q.h); }, kBatch,
   kLaunchTiles, false);
  for (int k = 0; k < g.count(); k++) {
    const int rc = ssim_launch(st, pairs, g.idx.data() + g.first[k], g.first[k + 1] - g.first[k], par, d_sum, nullptr, s);
    if (rc) return rc;
  }
  if (weights) {
    for (int i = 0; i < n; i++) {
      const int rc = odhip_ssim_weight(pairs[i].w, pairs[i].h, par, &weights[i]);
      if (rc) return rc;
    }
  }
  return odhip_check_launch();
}

extern "C" int odhip_ssim_terms(const odhip_metrics_pair *pair, double par, double *d_terms, odhip_stream stream) {
  if (!pair || !d_terms || !pair_ok(*pair) || !par_ok(par)) return ODHIP_EINVAL;
  ODHIP_CTX_OR_RETURN(ctx);
  MetricsState *st = odhip_ctx_state<MetricsState>(ctx, ODHIP_SLOT_METRICS);
  int rc = ssim_radius_check(st, pair->w, pair->h, par);
  if (rc) return rc;
  const int idx = 0;
  rc = ssim_launch(st, pair, &idx, 1, par, nullptr, d_terms, (hipStream_t)stream);
  return rc ? rc : odhip_check_launch();
}
