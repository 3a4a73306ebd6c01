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

   The host divides by the pixel count (PSNR) or by 64 x windows and samplemax^2 (PSNR-HVS-M). */
#include <math.h>
#include "../../include/daala_hip.h"
#include "od_ctx.cuh"
#include "od_lift.cuh"
#include "gen/od_csf_tables.h"

namespace {

constexpr int kChunks = 64;          /* partials per pair */
constexpr int kThreads = 256;
constexpr int kBatch = 32;           /* pairs per launch (kernel argument size) */

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

__device__ __forceinline__ int load_sample(const void *base, int fmt, int stride, int x, int y, int depth) {
  const long at = (long)y*stride + x;
  if (fmt == ODHIP_SAMPLE_U8) return static_cast<const uint8_t *>(base)[at];
  if (fmt == ODHIP_SAMPLE_U16) return static_cast<const uint16_t *>(base)[at];
  const int sh = 12 - depth;
  const int v = (static_cast<const int16_t *>(base)[at] + (1 << sh >> 1)) >> sh;
  return min(max(v, 0), (1 << depth) - 1);
}

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

/* the chunk partials of one batch, per context (one call sequence in flight per context) */
struct MetricsState {
  long long *part_sse = nullptr;
  double *part_hvs = nullptr;
  ~MetricsState() {
    if (part_sse) (void)hipFree(part_sse);
    if (part_hvs) (void)hipFree(part_hvs);
  }
};

bool fmt_ok(int fmt, int depth) {
  return (fmt == ODHIP_SAMPLE_U8 && depth == 8) || fmt == ODHIP_SAMPLE_U16 || fmt == ODHIP_SAMPLE_I16_12;
}

bool pair_ok(const odhip_metrics_pair &q) {
  return q.src && q.rec && q.w > 0 && q.h > 0 && q.w <= 65535 && q.h <= 65535 && q.src_stride >= q.w
   && q.rec_stride >= q.w && (q.depth == 8 || q.depth == 10 || q.depth == 12) && fmt_ok(q.src_fmt, q.depth)
   && fmt_ok(q.rec_fmt, q.depth) && q.csf >= ODHIP_CSF_Y && q.csf <= ODHIP_CSF_CR;
}

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
  if (!st->part_sse) ODHIP_TRY(hipMalloc(&st->part_sse, sizeof(long long)*kBatch*kChunks));
  if (!st->part_hvs) ODHIP_TRY(hipMalloc(&st->part_hvs, sizeof(double)*kBatch*kChunks));
  return ODHIP_SUCCESS;
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
    k_metrics<<<dim3(kChunks, (unsigned)m), kThreads, 0, s>>>(b, st->part_sse, st->part_hvs);
    k_metrics_sum<<<1, 64, 0, s>>>(m, flags, st->part_sse, st->part_hvs, d_sse ? d_sse + first : nullptr,
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
