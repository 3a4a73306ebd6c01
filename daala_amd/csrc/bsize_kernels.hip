/* bsize_kernels.hip - a frame's block sizes by activity masking: od_split_superblock
   (src/block_size_enc.c:331-456) of every 32x32 cell of a luma plane, on the device.

   The reference function is a pure function of a 44x44 window of the picture (the cell and
   OD_BLOCK_OFFSET = 6 samples around it, src/block_size_enc.h:50-51), the same window of an optional
   prediction and the quantiser; no cell depends on another.  Its frame-level wrapper
   (od_split_superblocks, src/encode.c:2381-2439) is stale, so the tiling is this library's: one call
   per 32x32 cell at a 32-sample pitch, samples outside the plane replicated from its edge, map values
   0..3 - a legal quadtree for every reader of d_bsize.

   One wavefront decides one cell (k_bsize_cell, one 64-lane workgroup, ~24 KB of LDS):
     window      the 44x44 samples, coordinates clamped, minus 128 (keyframe) - and again as
                 clamp(px - pred, -128, 127) for the residual's statistics of an inter cell
     statistics  od_compute_stats (:56-131): Sx2/Sxx2 -> Sx4/Sxx4 -> Var4/invVar4, Sx8/Sxx8 -> Var8/invVar8,
                 all lanes, integers; invVar* come from the picture, Var* from the residual
     noise       the 90 region averages (od_noise_var4x4 :191-212, od_noise_var8x8 :266-288): 64 + 16 + 4 + 1
                 regions of 4x4 variances, 4 + 1 of 8x8 ones
     terms       the 2082 log2 terms of the 90 regions (od_psy_var4x4 :225-246, od_psy_var8x8 :291-313), all
                 lanes, operation by operation as the reference evaluates them: int product, int -> float,
                 float division by 16384, float 1 +, double M_LOG2E*log() - for x a power of two the host libm's
                 own value from a 14-entry table (bsize_pow2)
     chains      one lane per region adds its terms in the reference's row-major order,
                 psy = (float)((double)psy + term) - never reordered; the 441-term chain of the 32x32 region is
                 the critical path
     decision    the three bottom-up comparisons (:374-455) with the reference's mix of float and double

   libm margin.  The device's log is OCML's, the reference's is glibc's; everything else is IEEE arithmetic
   that both sides round alike (-ffp-contract=off).  A differing last bit of a term changes a sum only where
   (double)psy + term lies next to a float rounding midpoint, so every accumulation step measures its
   distance to the two midpoints around it; a cell with a step inside kBsizeMarginUlps double ulps of one is
   LISTED, and odhip_bsize_resolve decides the listed cells again on the host with libm (bsize_cell on one
   "lane": the same code, compiled for the host) and overwrites what the device wrote.  The host path is
   public too: odhip_bsize_decide_host / odhip_bsize_terms_host make no HIP call. */
#include <limits.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "../../include/daala_hip.h"
#include "od_buf.cuh"
#include "od_ctx.cuh"

namespace {

constexpr int kCell = 32;                 /* a cell: the reference's 32x32 superblock */
constexpr int kBorder = 6;                /* OD_BLOCK_OFFSET: 2*OD_MAX_OVERLAP samples on every side */
constexpr int kWin = kCell + 2*kBorder;   /* 44 = 2*OD_SIZE2_SUMS */
constexpr int kS2 = 22;                   /* OD_SIZE2_SUMS */
constexpr int kS4 = 21;                   /* OD_SIZE4_SUMS */
constexpr int kS8 = 9;                    /* OD_SIZE8_SUMS */
constexpr int kRegions = ODHIP_BSIZE_TERMS;
constexpr int kTerms = 64*9 + 16*25 + 4*121 + 441 + 4*25 + 81;   /* 2082 */
constexpr int kMaxDim = 8192;
constexpr int kFramesPerLaunch = 16;      /* their scalars travel in the kernel's arguments */

/* The margin, in ulps of the double sum s = (double)psy + term, inside which a float rounding midpoint
   makes a step undecidable on the device.  Both sides compute term = fl(M_LOG2E * L) from the same double
   x (x is a float, exactly representable), L their library's log(x):
     glibc's log is within 1 ulp of the true value (its documented bound on x86-64), OCML's double log
     within 3 ulp (the OpenCL bound it is built to; HIP's own table states 1), so the two L differ by at most
     4 ulp(L);
     times M_LOG2E < 1.4427 that is at most 5.8 ulp(L) <= 5.8 ulp(term), since term >= L > 0 (or both are 0);
     each side then rounds the product once: + 2 * 0.5 ulp(term);
     s = psy + term >= term, so ulp(term) <= ulp(s), and each side rounds the sum once: + 2 * 0.5 ulp(s).
   Total: under 7.8 ulp(s), rounded up to 8.  ulp(s) <= 2^-52 * s. */
constexpr double kBsizeMarginUlps = 8.;
constexpr double kUlp = 2.220446049250313e-16;   /* 2^-52 */

struct BsizeScalars {
  double lambda;   /* psy_lambda (:346) */
  double cg4;      /* OD_CG4, less the inter adjustment (:352, :361) */
  double cg8;      /* OD_CG8, less the inter adjustment (:353, :362) */
};

/* The scalars of one frame, on the host: a double sqrt and two double products. */
BsizeScalars bsize_scalars(int q, bool inter) {
  BsizeScalars s;
  s.lambda = q ? 6*sqrt((double)(1 << 4)/q) : 6;
  s.cg4 = 15.943f/6;
  s.cg8 = 16.7836f/6;
  if (inter) {
    const int over = (q >> 4) - 40 > 0 ? (q >> 4) - 40 : 0;
    s.cg4 -= .01*over;
    s.cg8 -= .005*over;
  }
  return s;
}

/* Everything one cell needs between its phases: LDS on the device, the stack on the host. */
struct BsizeWork {
  union {
    struct {
      int s2x[kS2*kS2];
      int s2xx[kS2*kS2];
      int s4x[kS4*kS4];
      int s4xx[kS4*kS4];
    } sum;                  /* dead once Var / invVar are written */
    double term[kTerms];
  } u;
  int var4[kS4*kS4];        /* of the residual (img_stats) */
  int inv4[kS4*kS4];        /* of the picture (psy_stats) */
  int var8[kS8*kS8];
  int inv8[kS8*kS8];
  int noise[kRegions];
  float psy[kRegions];
  signed char win[kWin*kWin];
  int listed;
};

/* Region r of the 90: which table, the top-left entry it starts at and its side in entries.
   0..63 4x4 blocks, 64..79 8x8, 80..83 16x16, 84 32x32 over Var4 (length 2*n - 1 plus od_overlap_var4x4 =
   {1, 1, 2, 3} on every side, from OD_MAX_OVERLAP + y/2 - overlap); 85..88 16x16, 89 32x32 over Var8
   (od_overlap_var8x8 = 1, from OD_MAX_OVERLAP_8 + y/4 - 1). */
struct Region {
  int is8;
  int y0;
  int x0;
  int side;
  int first;    /* its first term among the 2082 */
};

__host__ __device__ inline Region bsize_region(int r) {
  Region g;
  g.is8 = r >= 85;
  if (r < 64) {
    g.side = 3; g.y0 = 2 + 2*(r >> 3); g.x0 = 2 + 2*(r & 7); g.first = 9*r;
  }
  else if (r < 80) {
    const int q = r - 64;
    g.side = 5; g.y0 = 2 + 4*(q >> 2); g.x0 = 2 + 4*(q & 3); g.first = 576 + 25*q;
  }
  else if (r < 84) {
    const int q = r - 80;
    g.side = 11; g.y0 = 1 + 8*(q >> 1); g.x0 = 1 + 8*(q & 1); g.first = 976 + 121*q;
  }
  else if (r == 84) {
    g.side = 21; g.y0 = 0; g.x0 = 0; g.first = 1460;
  }
  else if (r < 89) {
    const int q = r - 85;
    g.side = 5; g.y0 = 4*(q >> 1); g.x0 = 4*(q & 1); g.first = 1901 + 25*q;
  }
  else {
    g.side = 9; g.y0 = 0; g.x0 = 0; g.first = 2001;
  }
  return g;
}

/* The region of term t. */
__host__ __device__ inline int bsize_term_region(int t) {
  if (t < 576) return t/9;
  if (t < 976) return 64 + (t - 576)/25;
  if (t < 1460) return 80 + (t - 976)/121;
  if (t < 1901) return 84;
  if (t < 2001) return 85 + (t - 1901)/25;
  return 89;
}

/* The phases of a cell.  Each runs on `n` lanes, this one `lane`; the caller puts a barrier between
   two phases (the host runs them with n = 1). */

/* Sx2 / Sxx2 and Sx4 / Sxx4 of the window (:85-100). */
__host__ __device__ inline void bsize_sums2(BsizeWork *w, int lane, int n) {
  for (int e = lane; e < kS2*kS2; e += n) {
    const signed char *x = w->win + 2*(e/kS2)*kWin + 2*(e%kS2);
    const int a = x[0], b = x[1], c = x[kWin], d = x[kWin + 1];
    w->u.sum.s2x[e] = a + b + c + d;
    w->u.sum.s2xx[e] = a*a + b*b + c*c + d*d;
  }
}

__host__ __device__ inline void bsize_sums4(BsizeWork *w, int lane, int n) {
  for (int e = lane; e < kS4*kS4; e += n) {
    const int at = (e/kS4)*kS2 + e%kS4;
    const int *sx = w->u.sum.s2x + at;
    const int *sxx = w->u.sum.s2xx + at;
    w->u.sum.s4x[e] = sx[0] + sx[1] + sx[kS2] + sx[kS2 + 1];
    w->u.sum.s4xx[e] = sxx[0] + sxx[1] + sxx[kS2] + sxx[kS2 + 1];
  }
}

/* Var4 / invVar4 (:113-121) and, through Sx8 / Sxx8 (:101-112), Var8 / invVar8 (:122-130); want_var and
   want_inv say which of the two tables this window's statistics feed. */
__host__ __device__ inline void bsize_vars(BsizeWork *w, int lane, int n, bool want_var, bool want_inv) {
  for (int e = lane; e < kS4*kS4 + kS8*kS8; e += n) {
    int sx;
    int sxx;
    int shift;
    if (e < kS4*kS4) {
      sx = w->u.sum.s4x[e];
      sxx = w->u.sum.s4xx[e];
      shift = 4;
    }
    else {
      const int q = e - kS4*kS4;
      const int at = (2*(q/kS8) + 1)*kS4 + 2*(q%kS8) + 1;   /* off8 = OD_MAX_OVERLAP - 2*OD_MAX_OVERLAP_8 = 1 */
      const int *px = w->u.sum.s4x + at;
      const int *pxx = w->u.sum.s4xx + at;
      sx = px[0] + px[2] + px[2*kS4] + px[2*kS4 + 2];
      sxx = pxx[0] + pxx[2] + pxx[2*kS4] + pxx[2*kS4 + 2];
      shift = 6;
    }
    int var = (sxx - ((sx*sx) >> shift)) >> 5;
    const int var_floor = 4 + ((sx + (128 << shift)) >> 8);
    if (var < var_floor) var = var_floor;
    int *tv = e < kS4*kS4 ? w->var4 + e : w->var8 + (e - kS4*kS4);
    int *ti = e < kS4*kS4 ? w->inv4 + e : w->inv8 + (e - kS4*kS4);
    if (want_var) *tv = var;
    if (want_inv) *ti = 16384/var;
  }
}

__host__ __device__ inline void bsize_noise(BsizeWork *w, int lane, int n) {
  for (int r = lane; r < kRegions; r += n) {
    const Region g = bsize_region(r);
    const int *tab = g.is8 ? w->var8 : w->var4;
    const int pitch = g.is8 ? kS8 : kS4;
    int sum = 0;
    for (int i = 0; i < g.side; i++) {
      for (int j = 0; j < g.side; j++) sum += tab[(g.y0 + i)*pitch + g.x0 + j];
    }
    w->noise[r] = sum/(g.side*g.side);
  }
}

/* OD_LOG2(x) of x = 2^k, k = 0 .. kPow2 - 1, as the HOST's libm evaluates it: the kernel takes these terms from the
   table instead of OCML's log.  They are the structural case of the margin: a plane at its variance floor has
   noise*invVar == 16384 wherever the floor divides 16384, so x == 2 and the term is 1 - and a float plus 1 is an
   exact rounding tie whenever the sum needs one more bit.  On the bench content a quarter of all cells would be
   listed for such ties alone.  With the host's own value the device's term IS the reference's (the same
   expression, the same libm, the same argument: no error bound is involved), so the step needs no margin.
   x <= 1 + 2^27/16384: k <= 13. */
constexpr int kPow2 = 14;

struct BsizePow2 {
  double term[kPow2];
};

BsizePow2 bsize_pow2(void) {
  BsizePow2 t;
  for (int k = 0; k < kPow2; k++) t.term[k] = M_LOG2E*log((double)(1 << k));
  return t;
}

/* OD_LOG2(1 + noise*invVar/16384.f) of every entry of every region (:241-242, :308-309).  A term taken from the
   table is stored with its sign set (terms are never negative): bsize_chains adds its magnitude and skips the
   margin test of that step. */
__host__ __device__ inline void bsize_terms(BsizeWork *w, int lane, int n, const BsizePow2 &pow2) {
  for (int t = lane; t < kTerms; t += n) {
    const int r = bsize_term_region(t);
    const Region g = bsize_region(r);
    const int k = t - g.first;
    const int i = k/g.side;
    const int j = k - i*g.side;
    const int inv = g.is8 ? w->inv8[(g.y0 + i)*kS8 + g.x0 + j] : w->inv4[(g.y0 + i)*kS4 + g.x0 + j];
    const int prod = w->noise[r]*inv;
    const float ratio = (float)prod/16384.f;
    const float x = 1 + ratio;
    unsigned bits;
    memcpy(&bits, &x, sizeof(bits));
    const int e2 = (int)(bits >> 23) - 127;
    if ((bits & 0x7fffff) == 0 && e2 >= 0 && e2 < kPow2) w->u.term[t] = -pow2.term[e2];
    else w->u.term[t] = M_LOG2E*log((double)x);
  }
}

__host__ __device__ inline float bsize_float_from_bits(unsigned u) {
  float f;
  memcpy(&f, &u, sizeof(f));
  return f;
}

/* The accumulation of every region, one lane per chain, and OD_MAXF(psy/(count*count) - 1.f, 0) (:245,
   :312).  margin: kBsizeMarginUlps*2^-52 times the test hook's scale. */
__host__ __device__ inline void bsize_chains(BsizeWork *w, int lane, int n, double margin) {
  for (int r = lane; r < kRegions; r += n) {
    const Region g = bsize_region(r);
    const int count2 = g.side*g.side;
    const double *term = w->u.term + g.first;
    float psy = 0;
    bool near = false;
    for (int k = 0; k < count2; k++) {
      const bool exact = signbit(term[k]);     /* the host libm's own value (bsize_pow2) */
      const double s = (double)psy + fabs(term[k]);
      psy = (float)s;
      if (exact) continue;
      /* the midpoints between psy and its two float neighbours (exact in double; s >= 0) */
      unsigned bits;
      memcpy(&bits, &psy, sizeof(bits));
      const double up = .5*((double)psy + (double)bsize_float_from_bits(bits + 1));
      const double dn = psy > 0 ? .5*((double)psy + (double)bsize_float_from_bits(bits - 1)) : -1.;
      const double m = margin*s;
      near |= up - s <= m || s - dn <= m;
    }
    const float v = psy/count2 - 1.f;
    w->psy[r] = v > 0 ? v : 0;
    if (near) w->listed = 1;
  }
}

/* The three comparison levels (:374-455) from the 90 + 90 values, one lane.  Leaves psy[80..84] as the
   reference leaves psy16 / psy32: OD_MAXF with PSY8_FUDGE times the 8x8-based value, which stays in
   psy[85..89]. */
__host__ __device__ inline void bsize_levels(float *psy, const BsizeScalars &sc, unsigned char bsize[16]) {
  float dec8[16];
  float dec16[4];
  for (int i = 0; i < 4; i++) {
    for (int j = 0; j < 4; j++) {
      const float *p4 = psy + 2*i*8 + 2*j;
      const float psy4_avg = .25f*(p4[0] + p4[1] + p4[8] + p4[9]);
      const float gain4 = (float)(sc.cg4 - sc.lambda*psy4_avg);
      const float gain8 = (float)(sc.cg8 - sc.lambda*psy[64 + 4*i + j]);
      const bool big = gain8 >= gain4;
      bsize[4*i + j] = big ? 1 : 0;
      dec8[4*i + j] = big ? gain8 : gain4;
    }
  }
  for (int i = 0; i < 2; i++) {
    for (int j = 0; j < 2; j++) {
      const int r = 80 + 2*i + j;
      const float fudged = .5f*psy[85 + 2*i + j];
      psy[r] = psy[r] > fudged ? psy[r] : fudged;
      const float *d = dec8 + 2*i*4 + 2*j;
      const float gain8_avg = (float)(.25*(d[0] + d[1] + d[4] + d[5]));
      const float gain16 = (float)(16.9986f/6 - sc.lambda*psy[r]);
      if (gain16 >= gain8_avg) {
        bsize[(2*i)*4 + 2*j] = bsize[(2*i)*4 + 2*j + 1] = bsize[(2*i + 1)*4 + 2*j] = bsize[(2*i + 1)*4 + 2*j + 1] = 2;
        dec16[2*i + j] = gain16;
      }
      else dec16[2*i + j] = gain8_avg;
    }
  }
  const float fudged = .5f*psy[89];
  psy[84] = psy[84] > fudged ? psy[84] : fudged;
  const float gain16_avg = .25f*(dec16[0] + dec16[1] + dec16[2] + dec16[3]);
  const float gain32 = (float)(17.1f/6 - sc.lambda*psy[84]);
  if (gain32 >= gain16_avg) {
    for (int k = 0; k < 16; k++) bsize[k] = 3;
  }
}

inline int clampi(int lo, int x, int hi) {
  return x < lo ? lo : x > hi ? hi : x;
}

/* ---- the host path: one cell on one "lane", with libm ---------------------------------------- */

/* Rows y0 .. of a plane w x h; coordinates outside the plane are clamped (edge replication). */
struct HostPlane {
  const unsigned char *p;
  long stride;
  int y0;
  int w;
  int h;
  int at(int y, int x) const {
    return p[(clampi(0, y, h - 1) - y0)*stride + clampi(0, x, w - 1)];
  }
};

/* od_split_superblock of the cell whose top-left sample is (x, y).  pred: NULL for a keyframe.  Returns
   whether a device run of the cell would have been listed at `margin`. */
int bsize_cell_host(BsizeWork *w, const HostPlane &px, const HostPlane *pred, int x, int y,
 const BsizeScalars &sc, double margin, unsigned char bsize[16]) {
  w->listed = 0;
  for (int e = 0; e < kWin*kWin; e++) {
    w->win[e] = (signed char)(px.at(y - kBorder + e/kWin, x - kBorder + e%kWin) - 128);
  }
  bsize_sums2(w, 0, 1);
  bsize_sums4(w, 0, 1);
  bsize_vars(w, 0, 1, pred == nullptr, true);
  if (pred) {
    for (int e = 0; e < kWin*kWin; e++) {
      const int yy = y - kBorder + e/kWin;
      const int xx = x - kBorder + e%kWin;
      w->win[e] = (signed char)clampi(-128, px.at(yy, xx) - pred->at(yy, xx), 127);
    }
    bsize_sums2(w, 0, 1);
    bsize_sums4(w, 0, 1);
    bsize_vars(w, 0, 1, true, false);
  }
  bsize_noise(w, 0, 1);
  static const BsizePow2 pow2 = bsize_pow2();
  bsize_terms(w, 0, 1, pow2);
  bsize_chains(w, 0, 1, margin);
  bsize_levels(w->psy, sc, bsize);
  return w->listed;
}

/* ---- the kernel ------------------------------------------------------------------------------ */

struct BsizeArgs {
  unsigned char *bsize;
  const unsigned char *px;
  const unsigned char *pred;     /* nullptr: keyframe */
  int32_t *noise;                /* optional [cell][90], cell = (f*cells_y + cy)*cells_x + cx */
  float *psy;                    /* optional [cell][90] */
  unsigned *list;                /* [0]: the number of listed cells; [1 + i]: their indices */
  long bsize_frame_stride;
  long px_plane_stride;
  long pred_plane_stride;
  int bstride;
  int px_stride;
  int pred_stride;
  int w;
  int h;
  int frame0;                    /* the first frame of this launch */
  int perturb;
  double margin;
  BsizeScalars sc[kFramesPerLaunch];
  BsizePow2 pow2;
};

__global__ __launch_bounds__(64) void k_bsize_cell(BsizeArgs a) {
  __shared__ BsizeWork w;
  const int lane = threadIdx.x;
  const int cx = blockIdx.x;
  const int cy = blockIdx.y;
  const int f = a.frame0 + blockIdx.z;
  const unsigned char *px = a.px + f*a.px_plane_stride;
  const int x0 = cx*kCell - kBorder;
  const int y0 = cy*kCell - kBorder;
  if (lane == 0) w.listed = 0;
  for (int e = lane; e < kWin*kWin; e += 64) {
    const int y = min(max(y0 + e/kWin, 0), a.h - 1);
    const int x = min(max(x0 + e%kWin, 0), a.w - 1);
    w.win[e] = (signed char)((int)px[(long)y*a.px_stride + x] - 128);
  }
  __syncthreads();
  bsize_sums2(&w, lane, 64);
  __syncthreads();
  bsize_sums4(&w, lane, 64);
  __syncthreads();
  bsize_vars(&w, lane, 64, a.pred == nullptr, true);
  if (a.pred) {
    const unsigned char *pred = a.pred + f*a.pred_plane_stride;
    for (int e = lane; e < kWin*kWin; e += 64) {
      const int y = min(max(y0 + e/kWin, 0), a.h - 1);
      const int x = min(max(x0 + e%kWin, 0), a.w - 1);
      const int d = (int)px[(long)y*a.px_stride + x] - (int)pred[(long)y*a.pred_stride + x];
      w.win[e] = (signed char)min(max(d, -128), 127);
    }
    __syncthreads();
    bsize_sums2(&w, lane, 64);
    __syncthreads();
    bsize_sums4(&w, lane, 64);
    __syncthreads();
    bsize_vars(&w, lane, 64, true, false);
  }
  __syncthreads();
  bsize_noise(&w, lane, 64);
  __syncthreads();
  bsize_terms(&w, lane, 64, a.pow2);
  __syncthreads();
  bsize_chains(&w, lane, 64, a.margin);
  __syncthreads();
  __shared__ unsigned char decided[16];
  if (lane == 0) {
    bsize_levels(w.psy, a.sc[blockIdx.z], decided);
    if (w.listed) a.list[1 + atomicAdd(a.list, 1u)] = ((unsigned)f*gridDim.y + cy)*gridDim.x + cx;
  }
  __syncthreads();
  /* the test hook: a listed cell leaves the device deliberately wrong, so only the host's re-run can
     make it right */
  const bool wrong = w.listed && a.perturb;
  if (lane < 16) {
    unsigned char *map = a.bsize + f*a.bsize_frame_stride + (long)(cy*4 + (lane >> 2))*a.bstride + cx*4 + (lane & 3);
    *map = wrong ? (unsigned char)((decided[lane] + 1) & 3) : decided[lane];
  }
  if (a.noise) {
    const size_t cell = ((size_t)f*gridDim.y + cy)*gridDim.x + cx;
    for (int r = lane; r < kRegions; r += 64) {
      a.noise[cell*kRegions + r] = w.noise[r] + (wrong ? 1 : 0);
      a.psy[cell*kRegions + r] = wrong ? -1.f - w.psy[r] : w.psy[r];
    }
  }
}

/* ---- entry points ---------------------------------------------------------------------------- */

struct BsizeCall {
  unsigned char *bsize;
  int bstride;
  long bsize_frame_stride;
  const unsigned char *px;
  int px_stride;
  long px_plane_stride;
  const unsigned char *pred;
  int pred_stride;
  long pred_plane_stride;
  int nframes;
  int w;
  int h;
  const int32_t *quantizer;
};

/* The refusals every entry point shares; no HIP call. */
int bsize_check(const BsizeCall &c, bool device) {
  if (!c.bsize || !c.px || !c.quantizer || c.nframes < 1) return ODHIP_EINVAL;
  if (c.w <= 0 || c.h <= 0 || c.w % kCell || c.h % kCell || c.w > kMaxDim || c.h > kMaxDim) return ODHIP_EINVAL;
  if (c.bstride < c.w/8 || c.px_stride < c.w || (c.pred && c.pred_stride < c.w)) return ODHIP_EINVAL;
  for (int f = 0; f < c.nframes; f++) {
    if (c.quantizer[f] < 0) return ODHIP_EINVAL;
  }
  if (device && (long)c.nframes*(c.w/kCell)*(c.h/kCell) > INT_MAX - 1) return ODHIP_EINVAL;
  return ODHIP_SUCCESS;
}

/* The reference's psy_img == pred branch (:356): the same planes are no prediction. */
void bsize_same_planes(BsizeCall &c) {
  if (c.pred == c.px && c.pred_stride == c.px_stride && c.pred_plane_stride == c.px_plane_stride) c.pred = nullptr;
}

struct BsizeState {
  DeviceBuf<unsigned> list;   /* the count and the indices of the cells the last decide listed */
  long ncells = 0;            /* of that decide; 0: none since the last resolve */
};

double bsize_margin(const odhip_ctx *ctx) {
  return kBsizeMarginUlps*kUlp*(ctx->bsize_margin_scale > 0 ? ctx->bsize_margin_scale : 1.);
}

int bsize_launch(odhip_ctx *ctx, const BsizeCall &c, int32_t *d_noise, float *d_psy, hipStream_t s) {
  BsizeState *st = odhip_ctx_state<BsizeState>(ctx, ODHIP_SLOT_BSIZE);
  const long ncells = (long)c.nframes*(c.w/kCell)*(c.h/kCell);
  const int rc = st->list.grow((size_t)ncells + 1, s);
  if (rc) return rc;
  ODHIP_TRY(hipMemsetAsync(st->list.p, 0, sizeof(unsigned), s));
  BsizeArgs a;
  memset(&a, 0, sizeof(a));
  a.bsize = c.bsize;
  a.px = c.px;
  a.pred = c.pred;
  a.noise = d_noise;
  a.psy = d_psy;
  a.list = st->list.p;
  a.bsize_frame_stride = c.bsize_frame_stride;
  a.px_plane_stride = c.px_plane_stride;
  a.pred_plane_stride = c.pred_plane_stride;
  a.bstride = c.bstride;
  a.px_stride = c.px_stride;
  a.pred_stride = c.pred_stride;
  a.w = c.w;
  a.h = c.h;
  a.perturb = ctx->bsize_perturb;
  a.margin = bsize_margin(ctx);
  a.pow2 = bsize_pow2();
  for (int f0 = 0; f0 < c.nframes; f0 += kFramesPerLaunch) {
    const int nf = c.nframes - f0 < kFramesPerLaunch ? c.nframes - f0 : kFramesPerLaunch;
    a.frame0 = f0;
    for (int i = 0; i < nf; i++) a.sc[i] = bsize_scalars(c.quantizer[f0 + i], c.pred != nullptr);
    /* gridDim.y and .x are the cells of ONE frame in every launch: the kernel numbers its cells with them */
    k_bsize_cell<<<dim3(c.w/kCell, c.h/kCell, nf), 64, 0, s>>>(a);
    const int lrc = odhip_check_launch();
    if (lrc) return lrc;
  }
  st->ncells = ncells;
  return ODHIP_SUCCESS;
}

/* Decides the listed cells again on the host and overwrites the device's map bytes (and terms). */
int bsize_resolve(odhip_ctx *ctx, const BsizeCall &c, int32_t *d_noise, float *d_psy, hipStream_t s, int *relisted) {
  BsizeState *st = odhip_ctx_state<BsizeState>(ctx, ODHIP_SLOT_BSIZE);
  const int cells_x = c.w/kCell;
  const int cells_y = c.h/kCell;
  const long ncells = (long)c.nframes*cells_x*cells_y;
  if (st->ncells != ncells || st->list.cap < (size_t)ncells + 1) return ODHIP_EINVAL;   /* no decide of this call */
  ODHIP_TRY(hipStreamSynchronize(s));
  st->ncells = 0;
  unsigned count = 0;
  ODHIP_TRY(hipMemcpy(&count, st->list.p, sizeof(count), hipMemcpyDeviceToHost));
  *relisted = (int)count;
  if (!count) return ODHIP_SUCCESS;
  if ((long)count > ncells) return ODHIP_EFAULT;
  std::vector<unsigned> cells(count);
  ODHIP_TRY(hipMemcpy(cells.data(), st->list.p + 1, count*sizeof(unsigned), hipMemcpyDeviceToHost));
  std::vector<unsigned char> rows_px((size_t)kWin*c.w);
  std::vector<unsigned char> rows_pred(c.pred ? (size_t)kWin*c.w : 0);
  std::vector<BsizeWork> work(1);
  for (unsigned i = 0; i < count; i++) {
    if ((long)cells[i] >= ncells) return ODHIP_EFAULT;
    const int f = (int)(cells[i]/((unsigned)cells_x*cells_y));
    const int cy = (int)(cells[i]/cells_x)%cells_y;
    const int cx = (int)(cells[i]%cells_x);
    /* the rows of the cell's window that lie in the plane */
    const int r0 = clampi(0, cy*kCell - kBorder, c.h - 1);
    const int r1 = clampi(0, cy*kCell + kCell + kBorder - 1, c.h - 1);
    ODHIP_TRY(hipMemcpy2D(rows_px.data(), c.w, c.px + f*c.px_plane_stride + (long)r0*c.px_stride, c.px_stride,
     c.w, r1 - r0 + 1, hipMemcpyDeviceToHost));
    const HostPlane px = { rows_px.data(), c.w, r0, c.w, c.h };
    HostPlane pred = { rows_pred.data(), c.w, r0, c.w, c.h };
    if (c.pred) {
      ODHIP_TRY(hipMemcpy2D(rows_pred.data(), c.w, c.pred + f*c.pred_plane_stride + (long)r0*c.pred_stride,
       c.pred_stride, c.w, r1 - r0 + 1, hipMemcpyDeviceToHost));
    }
    unsigned char decided[16];
    (void)bsize_cell_host(work.data(), px, c.pred ? &pred : nullptr, cx*kCell, cy*kCell,
     bsize_scalars(c.quantizer[f], c.pred != nullptr), 0., decided);
    ODHIP_TRY(hipMemcpy2D(c.bsize + f*c.bsize_frame_stride + (long)cy*4*c.bstride + cx*4, c.bstride, decided, 4, 4, 4,
     hipMemcpyHostToDevice));
    if (d_noise) {
      ODHIP_TRY(hipMemcpy(d_noise + (size_t)cells[i]*kRegions, work[0].noise, sizeof(work[0].noise), hipMemcpyHostToDevice));
      ODHIP_TRY(hipMemcpy(d_psy + (size_t)cells[i]*kRegions, work[0].psy, sizeof(work[0].psy), hipMemcpyHostToDevice));
    }
  }
  return ODHIP_SUCCESS;
}

/* Argument checks, then the context: EINVAL needs no device, EIMPL only the context's flag. */
int bsize_enter(BsizeCall &c, odhip_ctx **ctx) {
  const int rc = bsize_check(c, true);
  if (rc) return rc;
  *ctx = odhip_ctx_current();
  if (!*ctx) return ODHIP_EINVAL;
  if ((*ctx)->fpr) return ODHIP_EIMPL;   /* od_split_superblock takes 8-bit samples only */
  bsize_same_planes(c);
  return ODHIP_SUCCESS;
}

}  // namespace

extern "C" int odhip_bsize_decide(uint8_t *d_bsize, int bstride, long bsize_frame_stride, const uint8_t *d_px,
 int px_stride, long px_plane_stride, const uint8_t *d_pred, int pred_stride, long pred_plane_stride, int nframes,
 int w, int h, const int32_t *quantizer, odhip_stream stream) {
  BsizeCall c = { d_bsize, bstride, bsize_frame_stride, d_px, px_stride, px_plane_stride, d_pred, pred_stride,
   pred_plane_stride, nframes, w, h, quantizer };
  odhip_ctx *ctx = nullptr;
  const int rc = bsize_enter(c, &ctx);
  return rc ? rc : bsize_launch(ctx, c, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int odhip_bsize_resolve(uint8_t *d_bsize, int bstride, long bsize_frame_stride, const uint8_t *d_px,
 int px_stride, long px_plane_stride, const uint8_t *d_pred, int pred_stride, long pred_plane_stride, int nframes,
 int w, int h, const int32_t *quantizer, odhip_stream stream, int *relisted) {
  BsizeCall c = { d_bsize, bstride, bsize_frame_stride, d_px, px_stride, px_plane_stride, d_pred, pred_stride,
   pred_plane_stride, nframes, w, h, quantizer };
  if (!relisted) return ODHIP_EINVAL;
  odhip_ctx *ctx = nullptr;
  const int rc = bsize_enter(c, &ctx);
  return rc ? rc : bsize_resolve(ctx, c, nullptr, nullptr, (hipStream_t)stream, relisted);
}

extern "C" int odhip_bsize_terms(int32_t *d_noise, float *d_psy, uint8_t *d_bsize, int bstride,
 long bsize_frame_stride, const uint8_t *d_px, int px_stride, long px_plane_stride, const uint8_t *d_pred,
 int pred_stride, long pred_plane_stride, int nframes, int w, int h, const int32_t *quantizer, odhip_stream stream,
 int *relisted) {
  BsizeCall c = { d_bsize, bstride, bsize_frame_stride, d_px, px_stride, px_plane_stride, d_pred, pred_stride,
   pred_plane_stride, nframes, w, h, quantizer };
  if (!d_noise || !d_psy || !relisted) return ODHIP_EINVAL;
  odhip_ctx *ctx = nullptr;
  int rc = bsize_enter(c, &ctx);
  if (rc) return rc;
  rc = bsize_launch(ctx, c, d_noise, d_psy, (hipStream_t)stream);
  return rc ? rc : bsize_resolve(ctx, c, d_noise, d_psy, (hipStream_t)stream, relisted);
}

extern "C" int odhip_bsize_terms_host(int32_t *noise, float *psy, uint8_t *bsize, int bstride, const uint8_t *px,
 int px_stride, const uint8_t *pred, int pred_stride, int w, int h, int quantizer, double margin_scale, int *listed) {
  BsizeCall c = { bsize, bstride, 0, px, px_stride, 0, pred, pred_stride, 0, 1, w, h, &quantizer };
  const int rc = bsize_check(c, false);
  if (rc) return rc;
  if (!noise != !psy) return ODHIP_EINVAL;
  bsize_same_planes(c);
  const BsizeScalars sc = bsize_scalars(quantizer, c.pred != nullptr);
  const double margin = kBsizeMarginUlps*kUlp*(margin_scale > 0 ? margin_scale : 1.);
  const HostPlane ppx = { px, px_stride, 0, w, h };
  const HostPlane ppred = { c.pred, pred_stride, 0, w, h };
  std::vector<BsizeWork> work(1);
  int nlisted = 0;
  for (int cy = 0; cy < h/kCell; cy++) {
    for (int cx = 0; cx < w/kCell; cx++) {
      unsigned char decided[16];
      nlisted += bsize_cell_host(work.data(), ppx, c.pred ? &ppred : nullptr, cx*kCell, cy*kCell, sc, margin, decided);
      for (int i = 0; i < 4; i++) memcpy(bsize + (long)(cy*4 + i)*bstride + cx*4, decided + 4*i, 4);
      if (noise) {
        const size_t cell = (size_t)cy*(w/kCell) + cx;
        memcpy(noise + cell*kRegions, work[0].noise, sizeof(work[0].noise));
        memcpy(psy + cell*kRegions, work[0].psy, sizeof(work[0].psy));
      }
    }
  }
  if (listed) *listed = nlisted;
  return ODHIP_SUCCESS;
}

extern "C" int odhip_bsize_decide_host(uint8_t *bsize, int bstride, const uint8_t *px, int px_stride,
 const uint8_t *pred, int pred_stride, int w, int h, int quantizer) {
  return odhip_bsize_terms_host(nullptr, nullptr, bsize, bstride, px, px_stride, pred, pred_stride, w, h, quantizer,
   1., nullptr);
}
