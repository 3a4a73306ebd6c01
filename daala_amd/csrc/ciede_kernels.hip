/* ciede_kernels.hip - CIEDE2000 on the device, as the reference's RD tool computes it (tools/dump_ciede2000.py: BT.709
   Y'CbCr -> sRGB -> linear -> XYZ -> Lab over scikit-image, then deltaE_ciede2000 with kL = 0.65, kC = 1, kH = 4).  The
   definition, operation by operation, is in daala_hip.h; tests/_ciede_ref.py restates it.  Everything is binary64, one
   IEEE operation per operation written here (-ffp-contract=off; `/` and __dsqrt_rn are correctly rounded), so only pow,
   cbrt, atan2, sin, cos and exp can differ from a host libm - and, within the last bits of the jump at 180 degrees, the
   side of it, which ciede_de00 takes from a cross product so that exactly opposite hues fall where exact arithmetic
   puts them.

   k_ciede      one workgroup per 32 x 32 pixel tile of one picture pair (a flat grid over pairs and tiles).  The six
                planes of the tile are staged in LDS as uint16 - whole row segments, adjacent lanes reading adjacent
                samples, in any ODHIP_SAMPLE_* format - and a lane owns the 2 x 2 pixels that share a 4:2:0 chroma
                sample: the chroma terms of R, G and B are computed once for the four (per pixel at 4:4:4).  The lane adds
                its four dE00 in raster order, the workgroup reduces in a fixed tree and leaves one partial per tile.
                Neighbouring pairs of a launch group with the same source picture (the five levels of a pipe step) form
                a RUN: the workgroup of the run's first pair computes the source's Lab once, keeps it in LDS, and walks
                the run's reconstructions, writing each pair's own partial; the workgroups of the other pairs of the run
                leave at once.  The partials, and so the sums, are the same bits with and without runs.
   k_ciede_lab  step 6 alone on Lab triples, through the same ciede_de00 (the test surface of the published table).
   k_metric_tile_sum (od_metric_launch.cuh) adds a pair's tile partials in a fixed order.
   LDS of k_ciede: 2 x 3 x 32 x 32 x 2 B samples + 3 x 1024 x 8 B source Lab + 2 KiB reduction = 38 KiB. */
#include <math.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <vector>
#include "../../include/daala_hip.h"
#include "od_ctx.cuh"
#include "od_metric_launch.cuh"
#include "od_sample.cuh"

namespace {

constexpr int kQuad = kTile/2;                        /* a lane owns pixels (2 qx .. 2 qx + 1, 2 qy .. 2 qy + 1) */
static_assert(kThreads == kQuad*kQuad, "k_ciede: a lane owns one 2 x 2 quad of the tile");
constexpr double kDeg = 57.29577951308232;            /* 180/pi */
constexpr double kRad = 0.017453292519943295;         /* pi/180 */
constexpr double k25p7 = 6103515625.;                 /* 25^7 */

struct Lab {
  double L, a, b;
};

/* what chroma adds to R, G and B: the products of step 2 */
struct ChromaTerms {
  double rcr, gcb, gcr, bcb;
};

__device__ __forceinline__ ChromaTerms chroma_terms(int cb, int cr, double s) {
  const double pb = ((double)cb - 128*s)/(224*s);
  const double pr = ((double)cr - 128*s)/(224*s);
  return ChromaTerms{1.28033*pr, 0.21482*pb, 0.38059*pr, 2.12798*pb};
}

/* sRGB to linear; a negative value takes the linear branch, and pow never sees one */
__device__ __forceinline__ double srgb_linear(double c) {
  if (c > 0.04045) return pow((c + 0.055)/1.055, 2.4);
  return c/12.92;
}

__device__ __forceinline__ double lab_f(double t) {
  if (t > 0.008856) return cbrt(t);
  return 7.787*t + 16./116.;
}

/* steps 1..5 of one pixel */
__device__ __forceinline__ Lab ycc_lab(int y, const ChromaTerms &c, double s) {
  const double yp = ((double)y - 16*s)/(219*s);
  const double r = srgb_linear(yp + c.rcr);
  const double g = srgb_linear((yp - c.gcb) - c.gcr);
  const double b = srgb_linear(yp + c.bcb);
  const double fx = lab_f(((0.412453*r + 0.357580*g) + 0.180423*b)/0.95047);
  const double fy = lab_f(((0.212671*r + 0.715160*g) + 0.072169*b)/1.0);
  const double fz = lab_f(((0.019334*r + 0.119193*g) + 0.950227*b)/1.08883);
  return Lab{116*fy - 16, 500*(fx - fy), 200*(fy - fz)};
}

__device__ __forceinline__ double pow7(double c) {
  const double c2 = c*c;
  const double c4 = c2*c2;
  return (c4*c2)*c;
}

/* atan2 in degrees, in [0, 360) */
__device__ __forceinline__ double hue(double b, double a) {
  const double h = atan2(b, a)*kDeg;
  return h < 0 ? h + 360 : h;
}

/* step 6: dE00 of (L1, a1, b1) and (L2, a2, b2) */
__device__ __forceinline__ double ciede_de00(const Lab &p, const Lab &q, double kL, double kC, double kH) {
  const double c1 = __dsqrt_rn(p.a*p.a + p.b*p.b);
  const double c2 = __dsqrt_rn(q.a*q.a + q.b*q.b);
  const double cb7 = pow7((c1 + c2)/2);
  const double g = 0.5*(1 - __dsqrt_rn(cb7/(cb7 + k25p7)));
  const double a1 = (1 + g)*p.a;
  const double a2 = (1 + g)*q.a;
  const double cp1 = __dsqrt_rn(a1*a1 + p.b*p.b);
  const double cp2 = __dsqrt_rn(a2*a2 + q.b*q.b);
  const double h1 = hue(p.b, a1);
  const double h2 = hue(q.b, a2);
  const double dl = q.L - p.L;
  const double dc = cp2 - cp1;
  const double cc = cp1*cp2;
  const double d = h2 - h1;
  /* |h2' - h1'| > 180: in exact arithmetic h2' - h1' is above 180 where the second hue lies clockwise of the first
     although its angle is the larger one, and below -180 the other way round.  The side comes from the sign of the
     cross product a1' b2 - b1 a2', not from comparing the rounded difference with 180: for exactly opposite hues,
     (a, b) against (-a, -b), both products are the same number and the cross product is exactly 0 - not above 180, as
     in exact arithmetic - where d is 180 give or take the last bit of two atan2 results.  (Two rows of the published
     table are such pairs.)  Away from the jump both tests agree; d beyond 90 keeps the sign's noise between nearly
     equal hues out of it. */
  const double cross = a1*q.b - p.b*a2;
  const bool wrap = (d > 90 && cross < 0) || (d < -90 && cross > 0);
  double dh = !wrap ? d : d > 0 ? d - 360 : d + 360;
  const double hs = h1 + h2;
  double hb = !wrap ? hs/2 : hs < 360 ? (hs + 360)/2 : (hs - 360)/2;
  if (cc == 0) {
    dh = 0;
    hb = hs;
  }
  const double dH = (2*__dsqrt_rn(cc))*sin((dh/2)*kRad);
  const double lb = (p.L + q.L)/2;
  const double cpb = (cp1 + cp2)/2;
  const double t = (((1 - 0.17*cos((hb - 30)*kRad)) + 0.24*cos((2*hb)*kRad)) + 0.32*cos((3*hb + 6)*kRad))
   - 0.20*cos((4*hb - 63)*kRad);
  const double u = (hb - 275)/25;
  const double dtheta = 30*exp(-(u*u));
  const double cpb7 = pow7(cpb);
  const double rc = 2*__dsqrt_rn(cpb7/(cpb7 + k25p7));
  const double l2 = (lb - 50)*(lb - 50);
  const double sl = 1 + (0.015*l2)/__dsqrt_rn(20 + l2);
  const double sc = 1 + 0.045*cpb;
  const double sh = 1 + (0.015*cpb)*t;
  const double rt = -sin((2*dtheta)*kRad)*rc;
  const double x = dl/(kL*sl);
  const double y = dc/(kC*sc);
  const double w = dH/(kH*sh);
  const double r = ((x*x + y*y) + w*w) + (rt*y)*w;
  /* (a NaN is not hidden) */
  return r < 0 ? 0 : __dsqrt_rn(r);
}

struct CieBatch {
  MetricTiles t;                                      /* one column */
  odhip_ciede_pair q[kBatch];
  int run[kBatch];                                    /* pairs of the run that pair i heads; 0: another pair heads it */
  int n;
};
static_assert(sizeof(CieBatch) <= 4000, "k_ciede's arguments fit the 4 KiB of kernel arguments");

/* the tile at luma (x0, y0) of one side of a pair: luma rows in whole segments, then both chroma planes */
__device__ __forceinline__ void stage(uint16_t (&s)[3][kTile][kTile], const void *const (&pl)[3], int fmt, int stride,
 int cstride, const odhip_ciede_pair &q, int x0, int y0, int tid) {
#pragma unroll
  for (int k = 0; k < kTile*kTile/kThreads; k++) {
    const int c = tid%kTile;
    const int r = tid/kTile + k*(kThreads/kTile);
    if (x0 + c < q.w && y0 + r < q.h) s[0][r][c] = (uint16_t)load_sample(pl[0], fmt, stride, x0 + c, y0 + r, q.depth);
  }
  const int cn = kTile >> q.cdec;
  const int cw = q.w >> q.cdec;
  const int ch = q.h >> q.cdec;
  for (int i = tid; i < 2*cn*cn; i += kThreads) {
    const int p = i/(cn*cn);
    const int r = (i - p*cn*cn)/cn;
    const int c = i%cn;
    const int x = (x0 >> q.cdec) + c;
    const int y = (y0 >> q.cdec) + r;
    if (x < cw && y < ch) s[1 + p][r][c] = (uint16_t)load_sample(pl[1 + p], fmt, cstride, x, y, q.depth);
  }
}

__global__ __launch_bounds__(kThreads) void k_ciede(CieBatch b, double *part, double *terms) {
  __shared__ uint16_t ss[3][kTile][kTile];
  __shared__ uint16_t sr[3][kTile][kTile];
  __shared__ double lab1[3][kTile*kTile];
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  const int e = find_entry(b.t.first, b.n, (int)blockIdx.x);
  const int run = b.run[e];
  if (run == 0) return;
  const odhip_ciede_pair &q = b.q[e];
  const int t = (int)blockIdx.x - b.t.first[e];
  const int ntx = (q.w + kTile - 1)/kTile;
  const int x0 = (t%ntx)*kTile;
  const int y0 = (t/ntx)*kTile;
  const int cdec = q.cdec;
  const double s = (double)(1 << (q.depth - 8));
  const int qx = 2*(tid%kQuad);
  const int qy = 2*(tid/kQuad);
  stage(ss, q.src, q.src_fmt, q.src_stride, q.src_cstride, q, x0, y0, tid);
  __syncthreads();
  /* the source's Lab, once for the run; pixel k of the quad at lab1[.][k*kThreads + tid], which only this lane reads */
  {
    ChromaTerms c = {};
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
      const int px = qx + (k & 1);
      const int py = qy + (k >> 1);
      if (x0 + px >= q.w || y0 + py >= q.h) continue;
      if (k == 0 || cdec == 0) c = chroma_terms(ss[1][py >> cdec][px >> cdec], ss[2][py >> cdec][px >> cdec], s);
      const Lab v = ycc_lab(ss[0][py][px], c, s);
      lab1[0][k*kThreads + tid] = v.L;
      lab1[1][k*kThreads + tid] = v.a;
      lab1[2][k*kThreads + tid] = v.b;
    }
  }
#pragma unroll 1
  for (int j = 0; j < run; j++) {
    const odhip_ciede_pair &qr = b.q[e + j];
    /* (the tree below has left every lane past its reads of the last reconstruction) */
    stage(sr, qr.rec, qr.rec_fmt, qr.rec_stride, qr.rec_cstride, qr, x0, y0, tid);
    __syncthreads();
    double sum = 0;
    ChromaTerms c = {};
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
      const int px = qx + (k & 1);
      const int py = qy + (k >> 1);
      if (x0 + px >= q.w || y0 + py >= q.h) continue;
      if (k == 0 || cdec == 0) c = chroma_terms(sr[1][py >> cdec][px >> cdec], sr[2][py >> cdec][px >> cdec], s);
      const Lab v2 = ycc_lab(sr[0][py][px], c, s);
      const Lab v1 = Lab{lab1[0][k*kThreads + tid], lab1[1][k*kThreads + tid], lab1[2][k*kThreads + tid]};
      const double de = ciede_de00(v1, v2, 0.65, 1., 4.);
      if (terms) terms[(size_t)(y0 + py)*q.w + (x0 + px)] = de;
      sum += de;
    }
    red[tid] = sum;
    __syncthreads();
    for (int k = kThreads/2; k > 0; k >>= 1) {
      if (tid < k) red[tid] += red[tid + k];
      __syncthreads();
    }
    if (tid == 0) part[b.t.first[e + j] + t] = red[0];
  }
}

__global__ __launch_bounds__(kThreads) void k_ciede_lab(const double *lab1, const double *lab2, long n, double kL, double kC,
 double kH, double *out) {
  const long i = (long)blockIdx.x*kThreads + threadIdx.x;
  if (i >= n) return;
  const Lab p = Lab{lab1[3*i], lab1[3*i + 1], lab1[3*i + 2]};
  const Lab q = Lab{lab2[3*i], lab2[3*i + 1], lab2[3*i + 2]};
  out[i] = ciede_de00(p, q, kL, kC, kH);
}

bool cie_fmt_ok(int fmt, int depth) {
  return fmt == ODHIP_SAMPLE_U8 ? depth == 8 : fmt == ODHIP_SAMPLE_U16 || fmt == ODHIP_SAMPLE_I16_12;
}

bool cie_pair_ok(const odhip_ciede_pair &q) {
  for (int i = 0; i < 3; i++) {
    if (!q.src[i] || !q.rec[i]) return false;
  }
  if (q.w < 1 || q.h < 1 || q.w > 65535 || q.h > 65535 || q.cdec < 0 || q.cdec > 1) return false;
  if (q.cdec && ((q.w | q.h) & 1)) return false;
  if (q.depth != 8 && q.depth != 10 && q.depth != 12) return false;
  if (!cie_fmt_ok(q.src_fmt, q.depth) || !cie_fmt_ok(q.rec_fmt, q.depth)) return false;
  const int cw = q.w >> q.cdec;
  return q.src_stride >= q.w && q.rec_stride >= q.w && q.src_cstride >= cw && q.rec_cstride >= cw;
}

/* the source picture of a pair, as a run sees it */
bool same_source(const odhip_ciede_pair &a, const odhip_ciede_pair &b) {
  return a.src[0] == b.src[0] && a.src[1] == b.src[1] && a.src[2] == b.src[2] && a.src_fmt == b.src_fmt
   && a.src_stride == b.src_stride && a.src_cstride == b.src_cstride && a.w == b.w && a.h == b.h && a.depth == b.depth
   && a.cdec == b.cdec;
}

bool source_before(const odhip_ciede_pair &a, const odhip_ciede_pair &b) {
  for (int i = 0; i < 3; i++) {
    if (a.src[i] != b.src[i]) return std::less<const void *>()(a.src[i], b.src[i]);
  }
  if (a.src_fmt != b.src_fmt) return a.src_fmt < b.src_fmt;
  if (a.src_stride != b.src_stride) return a.src_stride < b.src_stride;
  if (a.src_cstride != b.src_cstride) return a.src_cstride < b.src_cstride;
  if (a.w != b.w) return a.w < b.w;
  if (a.h != b.h) return a.h < b.h;
  if (a.depth != b.depth) return a.depth < b.depth;
  return a.cdec < b.cdec;
}

long cie_tiles(int w, int h) {
  return (long)((w + kTile - 1)/kTile)*((h + kTile - 1)/kTile);
}

struct CieScratch {
  DeviceBuf<double> part;          /* the tile partials of one launch group */
};

/* ODHIP_CIEDE_NO_RUNS (experiments build): every pair computes its source's Lab itself - the other side of the choice
   profiles/ciede.txt records */
bool cie_runs() {
  const char *e = ODHIP_EXP_ENV("ODHIP_CIEDE_NO_RUNS");
  return !(e && *e && *e != '0');
}

/* One launch group: the pairs pairs[idx[0 .. m)], m <= kBatch, pairs of one source next to each other; pair idx[i]'s sum
   goes to d_sum[idx[i]].  terms != NULL (the test surface, m == 1): the per-pixel values too. */
int cie_launch(CieScratch *st, const odhip_ciede_pair *pairs, const int *idx, int m, double *d_sum, double *terms,
 hipStream_t s) {
  CieBatch b;
  memset(&b, 0, sizeof(b));
  int tiles = 0;
  const bool runs = cie_runs();
  for (int i = 0; i < m; i++) {
    b.q[i] = pairs[idx[i]];
    b.t.out[i] = idx[i];
    b.t.first[i] = tiles;
    tiles += (int)cie_tiles(b.q[i].w, b.q[i].h);
  }
  for (int i = m; i <= kBatch; i++) b.t.first[i] = tiles;
  b.t.columns = 1;
  b.n = m;
  for (int i = 0; i < m;) {
    int r = 1;
    while (runs && i + r < m && same_source(b.q[i], b.q[i + r])) r++;
    b.run[i] = r;
    i += r;
  }
  const int rc = st->part.grow((size_t)tiles, s);
  if (rc) return rc;
  k_ciede<<<(unsigned)tiles, kThreads, 0, s>>>(b, st->part.p, terms);
  if (d_sum) metric_tile_sum(b.t, m, st->part.p, d_sum, s);
  return ODHIP_SUCCESS;
}

}  // namespace

extern "C" int odhip_ciede_score(double sum, int w, int h, double *score) {
  if (!score || w < 1 || h < 1) return ODHIP_EINVAL;
  *score = 45 - 20*log10(sum/((double)w*h));
  return ODHIP_SUCCESS;
}

extern "C" int odhip_ciede_prepare(int w, int h, int pairs) {
  if (w < 1 || h < 1 || w > 65535 || h > 65535 || pairs < 1) return ODHIP_EINVAL;
  ODHIP_CTX_OR_RETURN(ctx);
  return odhip_ctx_state<CieScratch>(ctx, ODHIP_SLOT_CIEDE)->part.reserve((size_t)std::min(pairs, kBatch)*cie_tiles(w, h));
}

extern "C" int odhip_ciede_pictures(const odhip_ciede_pair *pairs, int n, double *d_sum, odhip_stream stream) {
  if (n < 1 || !pairs || !d_sum) return ODHIP_EINVAL;
  for (int i = 0; i < n; i++) {
    if (!cie_pair_ok(pairs[i])) return ODHIP_EINVAL;
  }
  ODHIP_CTX_OR_RETURN(ctx);
  CieScratch *st = odhip_ctx_state<CieScratch>(ctx, ODHIP_SLOT_CIEDE);
  /* pairs of one source picture next to each other, in the call's order otherwise; a group takes up to kBatch pairs
     and, unless a single pair is larger, kLaunchTiles tiles */
  std::vector<int> idx((size_t)n);
  for (int i = 0; i < n; i++) idx[i] = i;
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return source_before(pairs[a], pairs[b]); });
  for (int first = 0; first < n;) {
    int m = 0;
    long tiles = 0;
    while (first + m < n && m < kBatch) {
      const long t = cie_tiles(pairs[idx[first + m]].w, pairs[idx[first + m]].h);
      if (m > 0 && tiles + t > kLaunchTiles) break;
      tiles += t;
      m++;
    }
    const int rc = cie_launch(st, pairs, idx.data() + first, m, d_sum, nullptr, (hipStream_t)stream);
    if (rc) return rc;
    first += m;
  }
  return odhip_check_launch();
}

extern "C" int odhip_ciede_terms(const odhip_ciede_pair *pair, double *d_terms, odhip_stream stream) {
  if (!pair || !d_terms || !cie_pair_ok(*pair)) return ODHIP_EINVAL;
  ODHIP_CTX_OR_RETURN(ctx);
  const int idx = 0;
  const int rc = cie_launch(odhip_ctx_state<CieScratch>(ctx, ODHIP_SLOT_CIEDE), pair, &idx, 1, nullptr, d_terms,
   (hipStream_t)stream);
  return rc ? rc : odhip_check_launch();
}

extern "C" int odhip_ciede_lab_terms(const double *d_lab1, const double *d_lab2, long n, double kL, double kC, double kH,
 double *d_out, odhip_stream stream) {
  if (!d_lab1 || !d_lab2 || !d_out || n < 1 || n > (1L << 30)) return ODHIP_EINVAL;
  if (!(kL > 0) || !(kC > 0) || !(kH > 0)) return ODHIP_EINVAL;
  k_ciede_lab<<<(unsigned)((n + kThreads - 1)/kThreads), kThreads, 0, (hipStream_t)stream>>>(d_lab1, d_lab2, n, kL, kC, kH,
   d_out);
  return odhip_check_launch();
}
