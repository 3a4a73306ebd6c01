/* me_kernels.hip - motion-vector grids by exhaustive block matching.

   The cost of a candidate is the reference's own block-matching cost (od_mv_est_bma_sad, src/mcenc.c:2224-2264):
   od_mc_predict1fmv8_c of one vector on the B x B block centred on a grid point (src/mcenc.c:2589-2611), then
   od_enc_sad of it against the source picture, clipped to the picture (src/mcenc.c:1615-1679).  The search over
   candidates is a fixed one (include/daala_hip.h): every full-pel offset within `range` in every slot, then
   three rounds of eight sub-pel neighbours, each won by the smallest key (cost, |mvx| + |mvy|, slot, mvy, mvx).
   A candidate is evaluated only where od_me_mv_ok (mc_walk.cuh) allows it, so every grid passes
   odhip_mc_check_grid at both decimations.  8-bit planes only.

   odhip_me_search2 has the two terms the reference's search has beside the luma SAD (include/daala_hip.h): the
   chroma planes in the cost (od_mv_est_bma_sad with OD_MC_USE_CHROMA: each chroma distortion >> 2) and SATD as the
   sub-pel metric (od_enc_satd).  odhip_me_search is a wrapper over it with neither flag.

   odhip_me_search3 searches coarse to fine (include/daala_hip.h): pyramids of the pictures and the reference planes by
   2 x 2 means (k_me_halve), then per slot a descent from level `levels` to 1 - a level is a luma plane of decimation
   j, every candidate on it full-pel - and stage 1 within `refine` of every slot's own centre; stage 2 is unchanged.
   With levels = 0 it calls odhip_me_search2.  Components reach 1223 eighth-pels, which the key (me_key) holds.

   One family of kernels, one 256-lane block per grid point and picture each, built from one set of parts:
     k_me_fullpel<LG, CH, LV>  stage 1.  Per slot it stages the clamped (B + 2 range)^2 window and the source block in
                       LDS (stage_slide_window, stage_block); a lane owns four neighbouring offsets of one row of the
                       search square and slides the block over them (slide_sad) with v_qsad_pk_u16_u8 (v_sad_u8 under a
                       byte mask, clip_masks, where the picture edge cuts a group of four columns); the packed 16-bit
                       sums are flushed to 32 bits before they can overflow; the key is reduced across the block
                       (block_min_key), so the winner does not depend on the lane.
                       CH = kNoChroma: the keys come straight from a lane's four sums.
                       CH = k444 / k420: the luma pass, then one pass per chroma plane, all into one LDS array of
                       per-offset distortions (the three plane sums stay apart until the >> 2), then the keys.  At
                       4:2:0 an odd luma offset is a chroma half-pel: the four phase planes (fx, fy in {0, 4}) of the
                       chroma window are built once per block, slot and plane with mc_hpass / mc_vpass, and a lane
                       slides over four offsets of one parity.  Stage 1 is a SAD search under either metric.
                       LV = kPlain: round the zero vector, odhip_me_search2's launches.  LV = 0 .. 2: a level of the
                       coarse-to-fine search, every slot round its own centre (MeArgs.centre), on the planes of pyramid
                       level LV, which it is handed as the job's planes; LV > 0 is luma only, its blocks are B >> LV
                       (one group of four columns at 4 x 4), and it writes per-slot winners instead of the grid.  A
                       coarse level keeps one block per point with the slots one after the other, like level 0: the
                       stagers and the key minimum stride by the block's 256 lanes, so several points per block would
                       fork them; what that costs is in profiles/me_hier.txt.
     k_me_halve        one halving of planes: a lane reads 8 bytes of two lines, writes four samples.
     k_me_level_sad    D_level of listed candidates straight from the level's planes (odhip_me_costs3, test surface).
     k_me_subpel<LG, FLAGGED>  stage 2: stages the winner's window, one sample wider on every side, and runs the
                       rounds (me_rounds): per candidate and plane the two filter passes of mc_filter.cuh from LDS and
                       a block-wide sum (plane_dist).  FLAGGED = false is the search without flags: one plane, SAD,
                       one window in LDS, no Hadamard code.  FLAGGED = true stages all three planes and reads the
                       planes and the metric from the flags at run time; under SATD a lane holds one row of an 8x8
                       (4x4) tile of differences, the horizontal butterflies run in registers, the vertical ones across
                       8 (4) lanes.
     k_me_costs<LG>    the same candidate evaluation for listed candidates, the plane distortions apart: the test
                       surface of odhip_me_costs and odhip_me_costs2.  Its speed is not a criterion: it always takes
                       the three-plane LDS and the run-time metric, whatever the caller asks for.

   odhip_me_search_vbs makes a grid of mixed block sizes out of those searches (include/daala_hip.h): per size the
   uniform search and odhip_mc_predict_planes of its grid, then three kernels of its own:
     k_me_cell_dist    the SAD of every size's prediction against the picture per 8x8 cell, one pass, a lane a cell
     k_me_vbs_decide   a wave per 64x64 cell: the cells summed up the quadtree, the at most 21 decisions in one word
     k_me_vbs_grid     a lane per grid point: its flag and the size it takes its record from (me_vbs.cuh), the copy
   Its searches run under another legality predicate (od_me_mv_ok_cells, mc_walk.cuh: the point must suit a leaf of the
   largest size wherever one could read it).  The kernels take either as intervals worked out once per block
   (legal_axis), selected through MeArgs. */
#include <string.h>
#include "../../include/daala_hip.h"
#include "od_common.cuh"
#include "od_ctx.cuh"
#include "mc_walk.cuh"
#include "mc_filter.cuh"
#include "me_vbs.cuh"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads/64;
constexpr int kRangeMax = 32;
constexpr int kLevelsMax = 2;                        /* halvings of the coarse-to-fine search (odhip_me_search3) */
constexpr int kRefineMax = 8;                        /* its radius below the top level */
/* keeps the cost inside int32, for lambda and lambda_subpel alike: a tile's SATD is at most its maximal SAD (the
   8x8 Hadamard sum is <= 8 * 64 * 255, >> 3), so a plane's distortion is <= 64*64*255, chroma adds at most half of
   luma (2 * (D >> 2)): 8 * 1.5 * 64*64*255 + 2^20 * 2*(8*32 + 7) < 2^31 */
constexpr int kLambdaMax = 1 << 20;
/* the coarse-to-fine search reaches further: the top level's range 32 at level 2 is 8*(32 << 2) eighth-pels, every
   level below adds refine <= 8 steps of its own, 8*(2 + 1) eighth-pels each, and stage 2 seven more */
constexpr int kMvMax = 8*(kRangeMax << kLevelsMax) + kRefineMax*(16 + 8) + 7;
/* ... so its lambdas stop one bit earlier: 8 * 1.5 * 64*64*255 + 2^19 * 2*1223 < 2^31 (a coarse SAD << 2j is on the
   scale of the B x B block, so the distortion term is level 0's) */
constexpr int kLambdaMaxHier = 1 << 19;
static_assert(kMvMax == 1223 && 12ll*64*64*255 + (long long)kLambdaMaxHier*2*kMvMax < 1ll << 31, "cost in int32");
constexpr int kMvBias = 2048;                        /* |component| <= kMvMax */

/* luma and chroma of a job flat in one struct; the chroma half is null / 0 without ODHIP_ME_CHROMA */
struct MeArgs {
  const uint8_t *src;
  const uint8_t *ref[3];
  const uint8_t *csrc;           /* [2F] chroma pictures, all Cb then all Cr */
  const uint8_t *cref[3];
  odhip_mv_point *grid;
  uint32_t *cost;
  long long src_plane_stride;
  long long ref_plane_stride;
  long long csrc_plane_stride;
  long long cref_plane_stride;
  int src_stride;
  int ref_stride;
  int csrc_stride;
  int cref_stride;
  int w;                         /* coded size */
  int h;
  int pic_w;
  int pic_h;
  int nh;
  int nv;
  int npics;
  int nrefs;
  int range;
  int res;
  int lambda;                    /* stage 1's */
  int lambda_subpel;             /* stage 2's */
  int flags;
  int cdec;
  /* the coarse-to-fine search: per valid point and slot the centre of the level's candidates, the winner of the
     level above as (mvy << 16 | mvx & 0xffff) in full-resolution eighth-pels; not read at the top level */
  uint32_t *centre;
  int top;
  /* which predicate decides a candidate's legality (legal_axis): < 0 od_me_mv_ok at the kernel's block size; else
     od_me_mv_ok_cells at this log size, the largest leaf of a variable-block-size grid (odhip_me_search_vbs) */
  int legal_lg;
};

/* One axis of the job's legality predicate for one point, worked out once per block: od_me_mv_ok at the kernel's block
   size, or od_me_mv_ok_cells, asks od_mc_window_ok of at most two leaves, at dec 0 and dec 1, and each such test bounds
   the sample offset od_mc_scale_mv(mv, dec) >> 3 from both sides - so the predicate is two intervals, one per
   decimation. */
struct LegalAxis {
  int lo[2], hi[2];
};

__device__ inline LegalAxis legal_axis(const MeArgs &a, int v, int lg, int n) {
  int c[2];
  if (a.legal_lg < 0) {
    c[0] = v;
    c[1] = v - (1 << lg);
  }
  else {
    lg = a.legal_lg;
    const int m = (1 << lg) - 1;
    c[0] = v & ~m;
    c[1] = v & m ? -1 : c[0] - m - 1;
  }
  LegalAxis o;
#pragma unroll
  for (int dec = 0; dec < 2; dec++) {
    o.lo[dec] = -(1 << 30);
    o.hi[dec] = 1 << 30;
#pragma unroll
    for (int d = 0; d < 2; d++) {
      if (c[d] < 0 || c[d] >= n) continue;
      /* od_mc_window_ok: x0 = base + s - OD_MC_TOP >= -pad and x0 + blk + OD_MC_APRON <= (n << 3 >> dec) + pad */
      const int base = c[d] << 3 >> dec;
      o.lo[dec] = max(o.lo[dec], OD_MC_TOP - (OD_MC_BORDER >> dec) - base);
      o.hi[dec] = min(o.hi[dec], (n << 3 >> dec) + (OD_MC_BORDER >> dec) - (8 << lg >> dec) - OD_MC_APRON + OD_MC_TOP - base);
    }
  }
  return o;
}

__device__ inline bool legal_ok(const LegalAxis &l, int mv) {
  const int s0 = mv >> 3;
  const int s1 = od_mc_scale_mv(mv, 1) >> 3;
  return s0 >= l.lo[0] && s0 <= l.hi[0] && s1 >= l.lo[1] && s1 <= l.hi[1];
}

/* the grid point and picture of a search kernel's block, and the corner of the point's B x B luma block */
struct Point {
  int vx, vy, pic, bx, by;
};

template <int LG>
__device__ inline Point point_of(const MeArgs &a) {
  const int npx = (a.nh >> LG) + 1;
  Point p;
  p.vx = (int)(blockIdx.x%npx) << LG;
  p.vy = (int)(blockIdx.x/npx) << LG;
  p.pic = blockIdx.y;
  p.bx = 8*p.vx - (4 << LG);
  p.by = 8*p.vy - (4 << LG);
  return p;
}

__device__ inline size_t grid_at(const MeArgs &a, const Point &p) {
  return ((size_t)p.pic*(a.nv + 1) + p.vy)*(a.nh + 1) + p.vx;
}

/* the part of a block that lies inside the picture, in block coordinates; empty when x1 <= x0 or y1 <= y0 */
struct Clip {
  int x0, x1, y0, y1;
};

__device__ inline Clip clip_of(int bx, int by, int blk, int pic_w, int pic_h) {
  Clip c;
  c.x0 = max(0, -bx);
  c.x1 = min(blk, pic_w - bx);
  c.y0 = max(0, -by);
  c.y1 = min(blk, pic_h - by);
  if (c.x1 <= c.x0 || c.y1 <= c.y0) c.x0 = c.x1 = c.y0 = c.y1 = 0;
  return c;
}

/* (cost, |mvx| + |mvy|, slot, mvy, mvx) as one integer whose order is the lexicographic one.  Three 12-bit vector
   fields beside 32 bits of cost and the slot do not fit; but once |mvx| + |mvy| and mvy are equal, mvx is one of
   +-(|mvx| + |mvy| - |mvy|): its sign is all that is left to compare, and gives it back. */
__device__ inline unsigned long long me_key(int cost, int slot, int mvx, int mvy) {
  return (unsigned long long)(unsigned)cost << 27 | (unsigned long long)(abs(mvx) + abs(mvy)) << 15
   | (unsigned long long)slot << 13 | (unsigned long long)(mvy + kMvBias) << 1 | (unsigned long long)(mvx > 0);
}
__device__ inline int key_mvy(unsigned long long k) { return (int)(k >> 1 & 4095) - kMvBias; }
__device__ inline int key_mvx(unsigned long long k) {
  const int m = (int)(k >> 15 & 4095) - abs(key_mvy(k));
  return k & 1 ? m : -m;
}
__device__ inline int key_slot(unsigned long long k) { return (int)(k >> 13 & 3); }
__device__ inline uint32_t key_cost(unsigned long long k) { return (uint32_t)(k >> 27); }

__device__ inline int me_cost(int sad, int lambda, int mvx, int mvy) {
  return 8*sad + lambda*(abs(mvx) + abs(mvy));
}

__device__ inline void write_point(const MeArgs &a, const Point &p, unsigned long long key) {
  const size_t at = grid_at(a, p);
  odhip_mv_point pt;
  pt.mvx = key_mvx(key);
  pt.mvy = key_mvy(key);
  pt.valid = 1;
  pt.ref = (uint8_t)key_slot(key);
  pt.reserved = 0;
  a.grid[at] = pt;
  if (a.cost) a.cost[at] = key_cost(key);
}

/* The smallest key of the block, in lane 0; red holds one key per wave. */
__device__ inline unsigned long long block_min_key(unsigned long long best, unsigned long long *red) {
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long other = __shfl_xor(best, d);
    best = other < best ? other : best;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kWaves; i++) best = red[i] < best ? red[i] : best;
  }
  return best;
}

/* the n x n source block as rows of n bytes; coordinates outside the picture are clamped (the clip rectangle keeps
   those samples out of every sum) */
__device__ inline void stage_block(uint8_t *blk, int n, const uint8_t *src, int stride, int bx, int by, int pic_w,
 int pic_h) {
  for (int e = threadIdx.x; e < n*n; e += kThreads) {
    const int x = min(max(bx + e%n, 0), pic_w - 1);
    const int y = min(max(by + e/n, 0), pic_h - 1);
    blk[e] = src[(size_t)y*stride + x];
  }
}

/* n x n bytes of a plane from (x0, y0), coordinates clamped to the plane: the reference's replicated border */
__device__ inline void stage_window(uint8_t *win, int n, const uint8_t *ref, int stride, int x0, int y0, int w,
 int h) {
  for (int e = threadIdx.x; e < n*n; e += kThreads) {
    const int x = min(max(x0 + e%n, 0), w - 1);
    const int y = min(max(y0 + e/n, 0), h - 1);
    win[e] = ref[(size_t)y*stride + x];
  }
}

__host__ __device__ inline int plane_sz(int n, int d) { return (n + (1 << d) - 1) >> d; }

/* picture, reference plane and geometry of plane pl (0 luma, 1 Cb, 2 Cr) of picture pic in slot */
struct PlaneOf {
  const uint8_t *src;
  const uint8_t *ref;
  int src_stride, ref_stride;
  int w, h, pic_w, pic_h;        /* plane and picture size at the plane's decimation */
  int d;
};

__device__ inline PlaneOf plane_of(const MeArgs &a, int pl, int pic, int slot) {
  PlaneOf o;
  if (!pl) {
    o.src = a.src + pic*a.src_plane_stride;
    o.ref = a.ref[slot] + pic*a.ref_plane_stride;
    o.src_stride = a.src_stride;
    o.ref_stride = a.ref_stride;
    o.d = 0;
  }
  else {
    const long long at = (long long)(pl - 1)*a.npics + pic;
    o.src = a.csrc + at*a.csrc_plane_stride;
    o.ref = a.cref[slot] + at*a.cref_plane_stride;
    o.src_stride = a.csrc_stride;
    o.ref_stride = a.cref_stride;
    o.d = a.cdec;
  }
  o.w = a.w >> o.d;
  o.h = a.h >> o.d;
  o.pic_w = plane_sz(a.pic_w, o.d);
  o.pic_h = plane_sz(a.pic_h, o.d);
  return o;
}

/* One row of the search square slid over a block: the SADs of four neighbouring window offsets (dwords q .. of the
   window rows from row0 on, wd dwords apart) against the block's rows y0 .. y1 of G dwords, under the byte masks of
   the clip rectangle. */
template <int G>
__device__ inline void slide_sad(const uint32_t *win, int wd, int row0, int q, const uint32_t *blk,
 const uint32_t (&mask)[G], int y0, int y1, uint32_t (&sad)[4]) {
  unsigned long long acc = 0;                /* four packed 16-bit sums */
  int pending = 0;                           /* quad SADs in acc: each adds at most 4*255 */
#pragma unroll
  for (int k = 0; k < 4; k++) sad[k] = 0;
  for (int j = y0; j < y1; j++) {
    const uint32_t *wrow = &win[(j + row0)*wd + q];
    const uint32_t *srow = &blk[j*G];
    uint32_t lo = wrow[0];
#pragma unroll
    for (int g = 0; g < G; g++) {
      const uint32_t hi = wrow[g + 1];
      const unsigned long long both = (unsigned long long)hi << 32 | lo;
      if (mask[g] == ~0u) {
        acc = __builtin_amdgcn_qsad_pk_u16_u8(both, srow[g], acc);
        pending++;
      }
      else if (mask[g]) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          sad[k] = __builtin_amdgcn_sad_u8((uint32_t)(both >> 8*k) & mask[g], srow[g] & mask[g], sad[k]);
        }
      }
      lo = hi;
    }
    if (pending > 64 - G) {                  /* 64 quad SADs are the most 16 bits hold */
#pragma unroll
      for (int k = 0; k < 4; k++) sad[k] += (uint32_t)(acc >> 16*k) & 0xffff;
      acc = 0;
      pending = 0;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) sad[k] += (uint32_t)(acc >> 16*k) & 0xffff;
}

/* which bytes of each group of four columns are inside the clip rectangle */
template <int G>
__device__ inline void clip_masks(Clip c, uint32_t (&mask)[G]) {
#pragma unroll
  for (int g = 0; g < G; g++) {
    const int lo = min(max(c.x0 - 4*g, 0), 4);
    const int hi = min(max(c.x1 - 4*g, 0), 4);
    mask[g] = hi <= lo ? 0u : (hi == 4 ? ~0u : (1u << 8*hi) - 1) & ~((1u << 8*lo) - 1);
  }
}

/* the clamped window of full-pel offsets -r .. r round an n-wide block at (bx, by), rows of wd dwords */
__device__ inline void stage_slide_window(uint32_t *win, int n, int r, int wd, const uint8_t *ref, int stride, int bx,
 int by, int w, int h) {
  for (int e = threadIdx.x; e < (n + 2*r)*wd; e += kThreads) {
    const int y = min(max(by - r + e/wd, 0), h - 1);
    const int x0 = bx - r + 4*(e%wd);
    const uint8_t *row = ref + (size_t)y*stride;
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) v |= (uint32_t)row[min(max(x0 + b, 0), w - 1)] << 8*b;
    win[e] = v;
  }
}

/* ---- stage 1: every full-pel offset in every slot ---- */

enum { kNoChroma, k444, k420 };

/* The levels of the family.  kPlain: odhip_me_search2's stage 1, every slot round the zero vector.  LV >= 0: a level
   of the coarse-to-fine search (odhip_me_search3) - every slot round its own centre, on the planes of pyramid level
   LV, which the kernel is handed as the job's planes (block (bx >> LV, by >> LV) of size B >> LV, a step of
   8 << LV eighth-pels); LV > 0 is luma only and writes per-slot winners, LV = 0 is stage 1 within the refine radius. */
constexpr int kPlain = -1;

constexpr int quads_of(int rm) { return (2*rm + 1 + 3)/4; }   /* groups of four offsets along a row of the square */

/* LDS of k_me_fullpel with chroma in the cost, for B x B luma blocks and ranges up to RM */
template <int B_, int CH, int RM>
struct FullLds {
  static constexpr int CDEC = CH == k420;
  static constexpr int B = B_;
  static constexpr int G = B/4;              /* groups of four columns across the block */
  static constexpr int BC = B >> CDEC;
  static constexpr int GC = BC/4;
  static constexpr int kSide = 2*RM + 1;
  static constexpr int kQuads = quads_of(RM);
  static constexpr int WD = G + kQuads;      /* the widest window row, in dwords */
  static constexpr int WR = B + 2*RM;
  /* CDEC = 1: chroma integer offsets -kRcMax .. RM/2, a phase plane of P rows of PD dwords, built from a raw
     window of R x R samples */
  static constexpr int kRcMax = (RM + 1)/2;
  static constexpr int kNcoMax = RM/2 + kRcMax + 1;
  static constexpr int P = BC + kNcoMax - 1;
  static constexpr int PD = GC + (kNcoMax + 3)/4;
  static constexpr int R = P + kApron;
  static constexpr int kWinLuma = WR*WD;
  static constexpr int kWinPhase = CDEC ? 4*P*PD : 0;
  static constexpr int kWin = kWinLuma > kWinPhase ? kWinLuma : kWinPhase;   /* dwords */
  static constexpr int kRaw = CDEC ? (R*R + 3)/4 : 1;                        /* dwords */
  static constexpr int kMid = CDEC ? R*P : 2;                                /* int16 */
  unsigned long long red[kWaves];
  uint32_t win[kWin];
  uint32_t blk[B*G];
  uint32_t cblk[2][BC*GC];
  uint32_t dist[kSide*4*kQuads];             /* per-offset distortions, rows of 4 nq */
  uint32_t raw[kRaw];
  int16_t mid[kMid];
  uint8_t okx[4*kQuads];
  uint8_t oky[kSide];
};

/* ... and without: one window, the block, no per-offset array */
template <int B_, int RM>
struct FullLds<B_, kNoChroma, RM> {
  static constexpr int CDEC = 0;
  static constexpr int B = B_;
  static constexpr int G = B/4;
  static constexpr int BC = B;
  static constexpr int GC = G;
  unsigned long long red[kWaves];
  uint32_t win[(B + 2*RM)*(G + quads_of(RM))];
  uint32_t blk[B*G];
  uint8_t okx[4*quads_of(RM)];
  uint8_t oky[2*RM + 1];
};

template <int LG, int CH, int LV = kPlain>
__global__ __launch_bounds__(kThreads) void k_me_fullpel(MeArgs a) {
  constexpr int J = LV > 0 ? LV : 0;
  static_assert(J <= LG + 1 && (!J || CH == kNoChroma), "a coarse block is at least 4 x 4, and luma only");
  typedef FullLds<(8 << LG >> J), CH, (LV == 0 ? kRefineMax : kRangeMax)> L;
  constexpr int B = L::B, G = L::G, BC = L::BC, GC = L::GC, CDEC = L::CDEC;
  __shared__ L l;
  const Point p = point_of<LG>(a);
  const int bx = p.bx >> J;                  /* exact: B/2 >> J is at least 2 */
  const int by = p.by >> J;
  const int cbx = bx >> CDEC;
  const int cby = by >> CDEC;
  const int r = a.range;
  const int side = 2*r + 1;
  const int nq = (side + 3) >> 2;
  const int wd = G + nq;
  const int dp = 4*nq;                       /* row pitch of dist */
  const Clip c = clip_of(bx, by, B, a.pic_w, a.pic_h);
  const Clip cc = clip_of(cbx, cby, BC, plane_sz(a.pic_w, CDEC), plane_sz(a.pic_h, CDEC));
  stage_block((uint8_t *)l.blk, B, a.src + p.pic*a.src_plane_stride, a.src_stride, bx, by, a.pic_w, a.pic_h);
  if constexpr (CH != kNoChroma) {
    for (int pi = 0; pi < 2; pi++) {
      const PlaneOf o = plane_of(a, 1 + pi, p.pic, 0);
      stage_block((uint8_t *)l.cblk[pi], BC, o.src, o.src_stride, cbx, cby, o.pic_w, o.pic_h);
    }
  }
  /* which offsets of the square round the centre (cx, cy), in the level's samples, the point may take */
  auto mark_legal = [&](int cx, int cy) {
    /* (the intervals are worked out here, per call and axis, so that they are not live across a slot's passes) */
    {
      const LegalAxis lx = legal_axis(a, p.vx, LG, a.nh);
      for (int e = threadIdx.x; e < 4*nq; e += kThreads) l.okx[e] = e < side && legal_ok(lx, (8 << J)*(cx + e - r));
    }
    {
      const LegalAxis ly = legal_axis(a, p.vy, LG, a.nv);
      for (int e = threadIdx.x; e < side; e += kThreads) l.oky[e] = legal_ok(ly, (8 << J)*(cy + e - r));
    }
  };
  if constexpr (LV == kPlain) mark_legal(0, 0);
  uint32_t mask[G];
  clip_masks<G>(c, mask);
  unsigned long long best = ~0ull;
  for (int slot = 0; slot < a.nrefs; slot++) {
    /* the slot's centre in the level's samples: the winner of the level above, a multiple of two samples */
    int cx = 0;
    int cy = 0;
    uint32_t *centre = nullptr;
    if constexpr (LV != kPlain) {
      centre = &a.centre[((size_t)blockIdx.y*gridDim.x + blockIdx.x)*3 + slot];
      if (!a.top) {
        const uint32_t v = *centre;
        cx = (int16_t)(v & 0xffff) >> (3 + J);
        cy = (int16_t)(v >> 16) >> (3 + J);
      }
    }
    /* the key of offset (dxi - r, dyi - r) from the centre at distortion d, where the point may take it; a coarse
       distortion is put on the scale of the B x B block */
    auto offer = [&](const uint32_t &d, int dxi, int dyi) {
      if (!l.okx[dxi] || !l.oky[dyi]) return;
      const int mvx = (8 << J)*(cx + dxi - r);
      const int mvy = (8 << J)*(cy + dyi - r);
      const unsigned long long key = me_key(me_cost((int)(d << 2*J), a.lambda, mvx, mvy), slot, mvx, mvy);
      best = key < best ? key : best;
    };
    __syncthreads();                         /* the previous slot's lanes have read dist, the window and the marks */
    if constexpr (LV != kPlain) mark_legal(cx, cy);
    stage_slide_window(l.win, B, r, wd, a.ref[slot] + p.pic*a.ref_plane_stride, a.ref_stride, bx + cx, by + cy, a.w,
     a.h);
    __syncthreads();
    for (int t = threadIdx.x; t < side*nq; t += kThreads) {
      const int dyi = t/nq;
      const int q = t%nq;
      uint32_t sad[4];
      slide_sad<G>(l.win, wd, dyi, q, l.blk, mask, c.y0, c.y1, sad);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if constexpr (CH == kNoChroma) offer(sad[k], 4*q + k, dyi);
        else l.dist[dyi*dp + 4*q + k] = sad[k];
      }
    }
    if constexpr (CH != kNoChroma) {
      uint32_t cmask[GC];
      clip_masks<GC>(cc, cmask);
      for (int pi = 0; pi < 2; pi++) {
        const PlaneOf o = plane_of(a, 1 + pi, p.pic, slot);
        __syncthreads();                     /* the pass before has read the window */
        if constexpr (CH == k444) {
          /* chroma slides like luma; a lane owns the offsets it owned in the luma pass */
          stage_slide_window(l.win, BC, r, wd, o.ref, o.ref_stride, cbx + cx, cby + cy, o.w, o.h);
          __syncthreads();
          for (int t = threadIdx.x; t < side*nq; t += kThreads) {
            const int dyi = t/nq;
            const int q = t%nq;
            uint32_t sad[4];
            slide_sad<GC>(l.win, wd, dyi, q, l.cblk[pi], cmask, cc.y0, cc.y1, sad);
#pragma unroll
            for (int k = 0; k < 4; k++) l.dist[dyi*dp + 4*q + k] += sad[k] >> 2;
          }
        }
        else {
          /* the absolute luma offset x = cx + dx is the chroma vector 4 x eighth-pels: sample offset x >> 1 at phase
             4 (x & 1).  A centre is even (a multiple of 8 << 1 eighth-pels), so the phase follows dx and the sample
             offset is cx/2 + (dx >> 1) */
          const int rc = (r + 1) >> 1;
          const int nco = (r >> 1) + rc + 1; /* chroma sample offsets -rc .. r >> 1 from the centre's */
          const int nqc = (nco + 3) >> 2;
          const int np = BC + nco - 1;       /* rows and columns of a phase plane */
          const int pd = GC + nqc;
          const int rs = np + kApron;
          uint8_t *rawb = (uint8_t *)l.raw;
          stage_window(rawb, rs, o.ref, o.ref_stride, cbx + (cx >> 1) - rc - kTop, cby + (cy >> 1) - rc - kTop, o.w,
           o.h);
          __syncthreads();
          for (int px = 0; px < 2; px++) {
            /* both passes for every phase, as od_mc_predict1fmv8_c runs them, the first kept in int16 */
            for (int e = threadIdx.x; e < rs*np; e += kThreads) {
              l.mid[e] = (int16_t)mc_hpass<uint8_t>(&rawb[(e/np)*rs + e%np], 4*px);
            }
            __syncthreads();
            for (int py = 0; py < 2; py++) {
              uint8_t *plane = (uint8_t *)&l.win[(px + 2*py)*np*pd];
              for (int e = threadIdx.x; e < np*4*pd; e += kThreads) {
                const int x = e%(4*pd);
                const int y = e/(4*pd);
                plane[e] = x < np ? mc_vpass<uint8_t>(&l.mid[y*np + x], np, 4*py) : (uint8_t)0;
              }
            }
            __syncthreads();                 /* mid is free again; after px = 1 the planes are complete */
          }
          /* a lane slides over four offsets of one parity: neighbours in that parity's plane */
          for (int t = threadIdx.x; t < side*2*nqc; t += kThreads) {
            const int dyi = t/(2*nqc);
            const int px = t%(2*nqc)/nqc;
            const int q = t%nqc;
            const int dy = dyi - r;
            uint32_t sad[4];
            slide_sad<GC>(&l.win[(px + 2*(dy & 1))*np*pd], pd, (dy >> 1) + rc, q, l.cblk[pi], cmask, cc.y0, cc.y1,
             sad);
#pragma unroll
            for (int k = 0; k < 4; k++) {
              const int oi = 4*q + k;
              const int dx = 2*(oi - rc) + px;
              if (oi < nco && abs(dx) <= r) l.dist[dyi*dp + dx + r] += sad[k] >> 2;
            }
          }
        }
      }
      __syncthreads();
      for (int t = threadIdx.x; t < side*side; t += kThreads) offer(l.dist[t/side*dp + t%side], t%side, t/side);
    }
    if constexpr (LV > 0) {
      /* a coarse level descends per slot: the slot's winner is the centre of the level below */
      best = block_min_key(best, l.red);
      if (threadIdx.x == 0) *centre = (uint32_t)key_mvy(best) << 16 | ((uint32_t)key_mvx(best) & 0xffff);
      best = ~0ull;
    }
  }
  if constexpr (LV <= 0) {
    best = block_min_key(best, l.red);
    if (threadIdx.x == 0) write_point(a, p, best);
  }
}

/* One halving of a plane per block row of lanes (odhip_me_downsample): a lane reads eight neighbouring bytes of two
   lines - as one aligned 8-byte word each where the plane allows it, so a wave reads whole lines - and writes four
   output samples.  Read coordinates are clamped: an odd last row or column is replicated. */
__global__ __launch_bounds__(kThreads) void k_me_halve(uint8_t *dst, int dst_stride, long long dst_plane_stride,
 const uint8_t *src, int src_stride, long long src_plane_stride, int w, int h) {
  const int ow = (w + 1) >> 1;
  const int oh = (h + 1) >> 1;
  const int nq = (ow + 3) >> 2;
  const int t = (int)(blockIdx.x*kThreads + threadIdx.x);
  if (t >= nq*oh) return;
  const int y = t/nq;
  const int x0 = 4*(t%nq);
  const uint8_t *plane = src + blockIdx.y*src_plane_stride;
  const uint8_t *r0 = plane + (size_t)(2*y)*src_stride + 2*x0;
  const uint8_t *r1 = plane + (size_t)min(2*y + 1, h - 1)*src_stride + 2*x0;
  uint32_t in0[2], in1[2];
  if (2*x0 + 8 <= w && !(((uintptr_t)r0 | (uintptr_t)r1) & 7)) {
    const uint2 v0 = *(const uint2 *)r0;
    const uint2 v1 = *(const uint2 *)r1;
    in0[0] = v0.x, in0[1] = v0.y, in1[0] = v1.x, in1[1] = v1.y;
  }
  else {
    in0[0] = in0[1] = in1[0] = in1[1] = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const int at = min(2*x0 + b, w - 1) - 2*x0;
      in0[b >> 2] |= (uint32_t)r0[at] << 8*(b & 3);
      in1[b >> 2] |= (uint32_t)r1[at] << 8*(b & 3);
    }
  }
  uint32_t out = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t s0 = in0[k >> 1] >> 16*(k & 1);
    const uint32_t s1 = in1[k >> 1] >> 16*(k & 1);
    out |= (((s0 & 255) + (s0 >> 8 & 255) + (s1 & 255) + (s1 >> 8 & 255) + 2) >> 2) << 8*k;
  }
  uint8_t *d = dst + blockIdx.y*dst_plane_stride + (size_t)y*dst_stride + x0;
  if (x0 + 4 <= ow && !((uintptr_t)d & 3)) *(uint32_t *)d = out;
  else {
    for (int k = 0; k < min(4, ow - x0); k++) d[k] = (uint8_t)(out >> 8*k);
  }
}

/* ---- stage 2 and the test surface: one candidate at a time ---- */

/* LDS of one candidate evaluation over NP planes: per plane the window (one sample wider on every side than one
   vector's n + 5, rows WP apart whatever the plane's n) and the source block (rows n apart), one first filter pass */
template <int B, int NP>
struct CandLds {
  static constexpr int WP = B + kApron + 1;
  uint8_t win[NP][WP*WP];
  int16_t mid[(B + kApron)*B];
  uint8_t blk[NP][B*B];
  int red[kWaves];
};

/* Distortion of plane pl's prediction (block size n, phases (fx, fy), window offset (ox, oy)) against its source
   block inside the clip rectangle: SAD, or with satd od_enc_satd's dispatch on the clipped size - a w x w square
   of 4 takes the 4x4 Hadamard, (sum + 2) >> 2; of 8 .. 64 the 8x8 one per tile, (sum + 4) >> 3 per tile; anything
   else the SAD.  Without HAD the Hadamard code is not compiled and satd is ignored.  Every lane of the block calls
   it and gets the sum. */
template <bool HAD, int B, int NP>
__device__ inline int plane_dist(CandLds<B, NP> &l, int pl, int n, int ox, int oy, int fx, int fy, Clip c, bool satd) {
  constexpr int WP = CandLds<B, NP>::WP;
  const uint8_t *win = l.win[pl];
  const uint8_t *blk = l.blk[pl];
  if (fx | fy) {
    for (int e = threadIdx.x; e < (n + kApron)*n; e += kThreads) {
      l.mid[e] = (int16_t)mc_hpass<uint8_t>(&win[(oy + e/n)*WP + ox + e%n], fx);
    }
  }
  __syncthreads();
  auto diff = [&](int i, int j) {
    const int p = (fx | fy) ? (int)mc_vpass<uint8_t>(&l.mid[j*n + i], n, fy)
     : (int)win[(oy + j + kTop)*WP + ox + i + kTop];
    return p - (int)blk[j*n + i];
  };
  const int cw = c.x1 - c.x0;
  const int ch = c.y1 - c.y0;
  int acc = 0;
  if (HAD && satd && cw == ch && (cw == 4 || (cw >= 8 && !(cw & (cw - 1))))) {
    /* a lane holds one row of a tile; the tile's rows sit in neighbouring lanes of one wave */
    const int ts = cw == 4 ? 4 : 8;
    const int across = cw/ts;
    const int tasks = across*across*ts;
    for (int base = 0; base < tasks; base += kThreads) {
      const int t = base + threadIdx.x;
      const bool on = t < tasks;
      int d[8];
#pragma unroll
      for (int k = 0; k < 8; k++) d[k] = 0;
      if (on) {
        const int tile = t/ts;
        const int j = c.y0 + tile/across*ts + t%ts;
        const int i0 = c.x0 + tile%across*ts;
#pragma unroll
        for (int k = 0; k < 8; k++) {
          if (k < ts) d[k] = diff(i0 + k, j);
        }
      }
      /* a 4-wide row leaves d[4 .. 7] zero through the steps of 1 and 2 */
#pragma unroll
      for (int s = 1; s < 8; s <<= 1) {
        if (s < ts) {
#pragma unroll
          for (int k = 0; k < 8; k++) {
            if (!(k & s)) {
              const int u = d[k];
              const int v = d[k + s];
              d[k] = u + v;
              d[k + s] = u - v;
            }
          }
        }
      }
#pragma unroll
      for (int s = 1; s < 8; s <<= 1) {
        if (s < ts) {
#pragma unroll
          for (int k = 0; k < 8; k++) {
            const int other = __shfl_xor(d[k], s);
            d[k] = (threadIdx.x & s) ? other - d[k] : d[k] + other;
          }
        }
      }
      int sum = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) sum += abs(d[k]);
      for (int s = 1; s < ts; s <<= 1) sum += __shfl_xor(sum, s);
      /* the tile's rounding before tiles are added */
      if (on && t%ts == 0) acc += ts == 4 ? (sum + 2) >> 2 : (sum + 4) >> 3;
    }
  }
  else {
    for (int e = threadIdx.x; e < n*n; e += kThreads) {
      const int i = e%n;
      const int j = e/n;
      if (i < c.x0 || i >= c.x1 || j < c.y0 || j >= c.y1) continue;
      acc += abs(diff(i, j));
    }
  }
  for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
  if ((threadIdx.x & 63) == 0) l.red[threadIdx.x >> 6] = acc;
  __syncthreads();
  int sum = 0;
  for (int i = 0; i < kWaves; i++) sum += l.red[i];
  __syncthreads();                           /* red and mid are free again */
  return sum;
}

/* The rounds of stage 2 from the full-pel winner (mvx0, mvy0): its own key, then for step = 4 .. 1 << res the eight
   neighbours of the best so far at that step where od_me_mv_ok allows them.  eval(mvx, mvy) gives a candidate's key;
   every lane of the block calls it. */
template <int LG, class Eval>
__device__ inline unsigned long long me_rounds(const MeArgs &a, const Point &p, int mvx0, int mvy0, Eval eval) {
  unsigned long long best = eval(mvx0, mvy0);
  const LegalAxis lx = legal_axis(a, p.vx, LG, a.nh);
  const LegalAxis ly = legal_axis(a, p.vy, LG, a.nv);
  for (int step = 4; step >= 1 << a.res; step >>= 1) {
    const int cx = key_mvx(best);
    const int cy = key_mvy(best);
    for (int n = 0; n < 9; n++) {
      const int mvx = cx + (n%3 - 1)*step;
      const int mvy = cy + (n/3 - 1)*step;
      if (n == 4 || !legal_ok(lx, mvx) || !legal_ok(ly, mvy)) continue;
      const unsigned long long key = eval(mvx, mvy);
      best = key < best ? key : best;
    }
  }
  return best;
}

template <int LG, bool FLAGGED>
__global__ __launch_bounds__(kThreads) void k_me_subpel(MeArgs a) {
  constexpr int B = 8 << LG;
  constexpr int NP = FLAGGED ? 3 : 1;
  constexpr int WP = CandLds<B, NP>::WP;
  __shared__ CandLds<B, NP> l;
  const Point p = point_of<LG>(a);
  const odhip_mv_point pt = a.grid[grid_at(a, p)];
  const int slot = min((int)pt.ref, a.nrefs - 1);
  const int nplanes = FLAGGED && (a.flags & ODHIP_ME_CHROMA) ? 3 : 1;
  const bool satd = FLAGGED && (a.flags & ODHIP_ME_SATD);
  /* the full-pel winner (a multiple of 8) at each plane's decimation: every candidate of the rounds is within 7
     eighth-pels of it, scaled to dec = 1 within 4 - one sample either way */
  int fpx[NP], fpy[NP];
  Clip c[NP];
  /* (unrolled, so that the per-plane values stay in registers) */
#pragma unroll
  for (int pl = 0; pl < NP; pl++) {
    if (pl >= nplanes) continue;
    const PlaneOf o = plane_of(a, pl, p.pic, slot);
    const int n = B >> o.d;
    fpx[pl] = od_mc_scale_mv(pt.mvx, o.d) >> 3;
    fpy[pl] = od_mc_scale_mv(pt.mvy, o.d) >> 3;
    c[pl] = clip_of(p.bx >> o.d, p.by >> o.d, n, o.pic_w, o.pic_h);
    stage_block(l.blk[pl], n, o.src, o.src_stride, p.bx >> o.d, p.by >> o.d, o.pic_w, o.pic_h);
    stage_window(l.win[pl], WP, o.ref, o.ref_stride, (p.bx >> o.d) + fpx[pl] - kTop - 1,
     (p.by >> o.d) + fpy[pl] - kTop - 1, o.w, o.h);
  }
  __syncthreads();
  auto eval = [&](int mvx, int mvy) {
    int dist = 0;
#pragma unroll
    for (int pl = 0; pl < NP; pl++) {
      if (pl >= nplanes) continue;
      const int d = pl ? a.cdec : 0;
      const int sx = od_mc_scale_mv(mvx, d);
      const int sy = od_mc_scale_mv(mvy, d);
      const int v = plane_dist<FLAGGED>(l, pl, B >> d, (sx >> 3) - fpx[pl] + 1, (sy >> 3) - fpy[pl] + 1, sx & 7,
       sy & 7, c[pl], satd);
      dist += pl ? v >> 2 : v;
    }
    return me_key(me_cost(dist, a.lambda_subpel, mvx, mvy), slot, mvx, mvy);
  };
  const unsigned long long best = me_rounds<LG>(a, p, 8*fpx[0], 8*fpy[0], eval);
  if (threadIdx.x == 0) write_point(a, p, best);
}

/* does the candidate name a picture, a point, a slot and a vector that can be evaluated? */
__device__ inline bool cand_ok(const MeArgs &a, const odhip_me_cand &cd) {
  return cd.pic >= 0 && cd.pic < a.npics && cd.vx >= 0 && cd.vx <= a.nh && cd.vy >= 0 && cd.vy <= a.nv && cd.slot >= 0
   && cd.slot < a.nrefs && abs(cd.mvx) < 1 << 20 && abs(cd.mvy) < 1 << 20;
}

/* The test surface: nout (1 .. 3) values per candidate, the unshifted distortions of planes 0 .. nout - 1, 0 for
   a plane the flags leave out, all ~0 for a candidate that names nothing.  Not a hot path: one instantiation per
   size serves one plane and three, SAD and SATD. */
template <int LG>
__global__ __launch_bounds__(kThreads) void k_me_costs(MeArgs a, const odhip_me_cand *cands, int satd, int nout,
 uint32_t *out) {
  constexpr int B = 8 << LG;
  constexpr int WP = CandLds<B, 3>::WP;
  __shared__ CandLds<B, 3> l;
  const odhip_me_cand cd = cands[blockIdx.x];
  uint32_t *res = out + (size_t)nout*blockIdx.x;
  if (!cand_ok(a, cd)) {
    if ((int)threadIdx.x < nout) res[threadIdx.x] = ~0u;
    return;
  }
  const int bx = 8*cd.vx - B/2;
  const int by = 8*cd.vy - B/2;
  const int nplanes = a.flags & ODHIP_ME_CHROMA ? 3 : 1;
  for (int pl = 0; pl < nout; pl++) {
    if (pl >= nplanes) {
      if (threadIdx.x == 0) res[pl] = 0;
      continue;
    }
    const PlaneOf o = plane_of(a, pl, cd.pic, cd.slot);
    const int n = B >> o.d;
    const int sx = od_mc_scale_mv(cd.mvx, o.d);
    const int sy = od_mc_scale_mv(cd.mvy, o.d);
    const Clip c = clip_of(bx >> o.d, by >> o.d, n, o.pic_w, o.pic_h);
    stage_block(l.blk[pl], n, o.src, o.src_stride, bx >> o.d, by >> o.d, o.pic_w, o.pic_h);
    stage_window(l.win[pl], WP, o.ref, o.ref_stride, (bx >> o.d) + (sx >> 3) - kTop, (by >> o.d) + (sy >> 3) - kTop,
     o.w, o.h);
    __syncthreads();
    const int sum = plane_dist<true>(l, pl, n, 0, 0, sx & 7, sy & 7, c, satd != 0);
    if (threadIdx.x == 0) res[pl] = (uint32_t)sum;
  }
}

/* everything of a job but the search parameters and the outputs */
int check_planes(const odhip_me_job *job) {
  if (!job || !job->src || !od_mc_size_ok(job->coded_w, job->coded_h) || job->pic_w < 1
   || job->pic_w > job->coded_w || job->pic_h < 1 || job->pic_h > job->coded_h || job->npics < 1
   || job->npics > 65535 || job->nrefs < 1 || job->nrefs > 3 || job->log_size < 0
   || job->log_size > OD_MC_LOG_MVB_MAX || job->src_stride < job->pic_w || job->ref_stride < job->coded_w
   || job->src_plane_stride < (int64_t)job->src_stride*job->pic_h
   || job->ref_plane_stride < (int64_t)job->ref_stride*job->coded_h) {
    return ODHIP_EINVAL;
  }
  for (int r = 0; r < job->nrefs; r++) {
    if (!job->ref[r]) return ODHIP_EINVAL;
  }
  return ODHIP_SUCCESS;
}

/* the chroma half of a job2 */
int check_chroma(const odhip_me_job2 *job) {
  const odhip_me_job &y = job->luma;
  const int d = job->cdec;
  const int cw = (y.pic_w + (1 << d) - 1) >> d;
  const int ch = (y.pic_h + (1 << d) - 1) >> d;
  if (!job->csrc || job->csrc_stride < cw || job->cref_stride < y.coded_w >> d
   || job->csrc_plane_stride < (int64_t)job->csrc_stride*ch
   || job->cref_plane_stride < (int64_t)job->cref_stride*(y.coded_h >> d)) {
    return ODHIP_EINVAL;
  }
  for (int r = 0; r < y.nrefs; r++) {
    if (!job->cref[r]) return ODHIP_EINVAL;
  }
  return ODHIP_SUCCESS;
}

/* the planes of a job2 and what it adds to the search parameters */
int check_job2(const odhip_me_job2 *job) {
  if (!job) return ODHIP_EINVAL;
  const int rc = check_planes(&job->luma);
  if (rc) return rc;
  if ((job->flags & ~(ODHIP_ME_CHROMA | ODHIP_ME_SATD)) || job->cdec < 0 || job->cdec > 1 || job->lambda_subpel < 0
   || job->lambda_subpel > kLambdaMax) {
    return ODHIP_EINVAL;
  }
  return job->flags & ODHIP_ME_CHROMA ? check_chroma(job) : ODHIP_SUCCESS;
}

MeArgs args_of(const odhip_me_job2 *job2) {
  const odhip_me_job *job = &job2->luma;
  const bool chroma = (job2->flags & ODHIP_ME_CHROMA) != 0;
  MeArgs a;
  a.src = job->src;
  a.csrc = chroma ? job2->csrc : nullptr;
  for (int r = 0; r < 3; r++) {
    a.ref[r] = r < job->nrefs ? job->ref[r] : nullptr;
    a.cref[r] = chroma && r < job->nrefs ? job2->cref[r] : nullptr;
  }
  a.grid = job->grid;
  a.cost = job->cost;
  a.src_plane_stride = job->src_plane_stride;
  a.ref_plane_stride = job->ref_plane_stride;
  a.csrc_plane_stride = job2->csrc_plane_stride;
  a.cref_plane_stride = job2->cref_plane_stride;
  a.src_stride = job->src_stride;
  a.ref_stride = job->ref_stride;
  a.csrc_stride = job2->csrc_stride;
  a.cref_stride = job2->cref_stride;
  a.w = job->coded_w;
  a.h = job->coded_h;
  a.pic_w = job->pic_w;
  a.pic_h = job->pic_h;
  a.nh = job->coded_w >> 3;
  a.nv = job->coded_h >> 3;
  a.npics = job->npics;
  a.nrefs = job->nrefs;
  a.range = job->range;
  a.res = job->res;
  a.lambda = job->lambda;
  a.lambda_subpel = job2->lambda_subpel;
  a.flags = job2->flags;
  a.cdec = job2->cdec;
  a.centre = nullptr;
  a.top = 0;
  a.legal_lg = -1;
  return a;
}

/* a zeroed job2 round a luma job: no flags */
odhip_me_job2 job2_of(const odhip_me_job *job) {
  odhip_me_job2 job2;
  memset(&job2, 0, sizeof(job2));
  job2.luma = *job;
  return job2;
}

/* fn<LG> of the job's block size */
#define ME_BY_SIZE(lg, call) \
  do { \
    switch (lg) { \
      case 0: { constexpr int LG = 0; call; } break; \
      case 1: { constexpr int LG = 1; call; } break; \
      case 2: { constexpr int LG = 2; call; } break; \
      default: { constexpr int LG = 3; call; } break; \
    } \
  } while (0)

/* both costs entry points: nout values per candidate to d_out */
int me_costs(const odhip_me_job2 *job, const odhip_me_cand *d_cands, long n, int metric, int nout, uint32_t *d_out,
 odhip_stream stream) {
  const int rc = check_job2(job);
  if (rc) return rc;
  if (!d_cands || !d_out || n < 0 || n > 0x7fffffffL || metric < 0 || metric > 1) return ODHIP_EINVAL;
  ODHIP_CTX_OR_RETURN(ctx);
  if (ctx->fpr) return ODHIP_EIMPL;
  if (!n) return ODHIP_SUCCESS;
  const MeArgs a = args_of(job);
  ME_BY_SIZE(job->luma.log_size,
   (k_me_costs<LG><<<(unsigned)n, kThreads, 0, (hipStream_t)stream>>>(a, d_cands, metric, nout, d_out)));
  return odhip_check_launch();
}

/* ---- the coarse-to-fine search: pyramids, per-slot centres, levels ---- */

/* The test surface of the levels (odhip_me_costs3): D_level of one listed candidate per block, straight from the
   level's planes, which it is handed as the job's planes.  Not a hot path. */
__global__ __launch_bounds__(kThreads) void k_me_level_sad(MeArgs a, const odhip_me_cand *cands, int lg, int level,
 uint32_t *out) {
  __shared__ uint32_t red[kWaves];
  const odhip_me_cand cd = cands[blockIdx.x];
  if (!cand_ok(a, cd) || ((cd.mvx | cd.mvy) & ((8 << level) - 1))) {
    if (threadIdx.x == 0) out[blockIdx.x] = ~0u;
    return;
  }
  const int n = 8 << lg >> level;
  const int bx = (8*cd.vx - (4 << lg)) >> level;
  const int by = (8*cd.vy - (4 << lg)) >> level;
  const int ox = cd.mvx >> (3 + level);
  const int oy = cd.mvy >> (3 + level);
  const Clip c = clip_of(bx, by, n, a.pic_w, a.pic_h);
  const uint8_t *src = a.src + cd.pic*a.src_plane_stride;
  const uint8_t *ref = a.ref[cd.slot] + cd.pic*a.ref_plane_stride;
  uint32_t acc = 0;
  for (int e = threadIdx.x; e < n*n; e += kThreads) {
    const int i = e%n;
    const int j = e/n;
    if (i < c.x0 || i >= c.x1 || j < c.y0 || j >= c.y1) continue;
    const int x = min(max(bx + i + ox, 0), a.w - 1);
    const int y = min(max(by + j + oy, 0), a.h - 1);
    acc += abs((int)ref[(size_t)y*a.ref_stride + x] - (int)src[(size_t)(by + j)*a.src_stride + bx + i]);
  }
  for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kWaves; i++) acc += red[i];
    out[blockIdx.x] = acc;
  }
}

/* The private layout of a job3's scratch: per level j = 1 .. levels the source pictures' level ([F] planes of
   OD_PLANE_SZ(pic, j), rows packed), then per slot the reference planes' level ([F] planes of coded >> j); behind
   them one centre per valid point, picture and slot. */
struct HierLayout {
  size_t src[kLevelsMax + 1];
  size_t ref[kLevelsMax + 1][3];
  size_t centre;
  size_t bytes;
};

HierLayout layout_of(const odhip_me_job3 *job) {
  const odhip_me_job &y = job->base.luma;
  HierLayout o;
  memset(&o, 0, sizeof(o));
  size_t at = 0;
  auto take = [&](size_t n) {
    const size_t was = at;
    at += (n + 15) & ~(size_t)15;
    return was;
  };
  for (int j = 1; j <= job->levels; j++) {
    o.src[j] = take((size_t)plane_sz(y.pic_w, j)*plane_sz(y.pic_h, j)*y.npics);
    for (int r = 0; r < y.nrefs; r++) o.ref[j][r] = take((size_t)(y.coded_w >> j)*(y.coded_h >> j)*y.npics);
  }
  const size_t points = (size_t)((y.coded_w >> 3 >> y.log_size) + 1)*((y.coded_h >> 3 >> y.log_size) + 1)*y.npics;
  o.centre = take(points*3*sizeof(uint32_t));
  o.bytes = at;
  return o;
}

/* what a job3 adds to the planes of its job2: the levels and the scratch they need */
int check_levels(const odhip_me_job3 *job, bool with_scratch = true) {
  if (!job) return ODHIP_EINVAL;
  const int rc = check_job2(&job->base);
  if (rc) return rc;
  const int most = job->base.luma.log_size + 1 < kLevelsMax ? job->base.luma.log_size + 1 : kLevelsMax;
  if (job->levels < 0 || job->levels > most) return ODHIP_EINVAL;
  if (with_scratch && job->levels && (!job->scratch || job->scratch_bytes < layout_of(job).bytes)) return ODHIP_EINVAL;
  return ODHIP_SUCCESS;
}

int halve(uint8_t *dst, int dst_stride, long long dst_plane_stride, const uint8_t *src, int src_stride,
 long long src_plane_stride, int w, int h, int nplanes, hipStream_t s) {
  const int tasks = (((w + 1) >> 1) + 3)/4*((h + 1) >> 1);
  const dim3 g((unsigned)((tasks + kThreads - 1)/kThreads), (unsigned)nplanes);
  k_me_halve<<<g, kThreads, 0, s>>>(dst, dst_stride, dst_plane_stride, src, src_stride, src_plane_stride, w, h);
  return odhip_check_launch();
}

/* the job's planes at level j (j = 0: the job's own): what a level's kernel is handed */
MeArgs level_args(const odhip_me_job3 *job, const HierLayout &lay, int j) {
  MeArgs a = args_of(&job->base);
  a.centre = (uint32_t *)((uint8_t *)job->scratch + lay.centre);
  a.top = 0;
  if (!j) return a;
  uint8_t *base = (uint8_t *)job->scratch;
  a.pic_w = plane_sz(a.pic_w, j);
  a.pic_h = plane_sz(a.pic_h, j);
  a.w >>= j;
  a.h >>= j;
  a.src = base + lay.src[j];
  a.src_stride = a.pic_w;
  a.src_plane_stride = (long long)a.pic_w*a.pic_h;
  for (int r = 0; r < a.nrefs; r++) a.ref[r] = base + lay.ref[j][r];
  a.ref_stride = a.w;
  a.ref_plane_stride = (long long)a.w*a.h;
  return a;
}

/* levels 1 .. job->levels of the source pictures and of every slot's reference planes, each from the level below */
int build_pyramids(const odhip_me_job3 *job, const HierLayout &lay, hipStream_t s) {
  for (int j = 1; j <= job->levels; j++) {
    const MeArgs lo = level_args(job, lay, j - 1);
    const MeArgs hi = level_args(job, lay, j);
    int rc = halve((uint8_t *)hi.src, hi.src_stride, hi.src_plane_stride, lo.src, lo.src_stride, lo.src_plane_stride,
     lo.pic_w, lo.pic_h, lo.npics, s);
    for (int r = 0; r < lo.nrefs && !rc; r++) {
      rc = halve((uint8_t *)hi.ref[r], hi.ref_stride, hi.ref_plane_stride, lo.ref[r], lo.ref_stride,
       lo.ref_plane_stride, lo.w, lo.h, lo.npics, s);
    }
    if (rc) return rc;
  }
  return ODHIP_SUCCESS;
}

template <int LG, int LV>
void launch_coarse(const MeArgs &a, dim3 g, hipStream_t s) {
  if constexpr (LV <= LG + 1) k_me_fullpel<LG, kNoChroma, LV><<<g, kThreads, 0, s>>>(a);
}

/* everything odhip_me_search2 refuses */
int check_search2(const odhip_me_job2 *job2) {
  const int rc = check_job2(job2);
  if (rc) return rc;
  const odhip_me_job *job = &job2->luma;
  if (!job->grid || job->range < 0 || job->range > kRangeMax || job->res < 0 || job->res > 3 || job->lambda < 0
   || job->lambda > kLambdaMax) {
    return ODHIP_EINVAL;
  }
  return ODHIP_SUCCESS;
}

/* the launches of odhip_me_search2 on a checked job, under the legality predicate legal_lg names (MeArgs) */
int run_search2(const odhip_me_job2 *job2, int legal_lg, hipStream_t s) {
  const odhip_me_job *job = &job2->luma;
  MeArgs a = args_of(job2);
  a.legal_lg = legal_lg;
  const size_t points = (size_t)job->npics*(a.nh + 1)*(a.nv + 1);
  /* the points between the searched ones are all zero */
  ODHIP_TRY(hipMemsetAsync(job->grid, 0, points*sizeof(odhip_mv_point), s));
  if (job->cost) ODHIP_TRY(hipMemsetAsync(job->cost, 0, points*sizeof(uint32_t), s));
  const int lg = job->log_size;
  const dim3 g((unsigned)(((a.nh >> lg) + 1)*((a.nv >> lg) + 1)), (unsigned)job->npics);
  /* stage 1 is a SAD search under either metric: only chroma takes it off the luma-only instantiation */
  if (!(a.flags & ODHIP_ME_CHROMA)) ME_BY_SIZE(lg, (k_me_fullpel<LG, kNoChroma><<<g, kThreads, 0, s>>>(a)));
  else if (a.cdec) ME_BY_SIZE(lg, (k_me_fullpel<LG, k420><<<g, kThreads, 0, s>>>(a)));
  else ME_BY_SIZE(lg, (k_me_fullpel<LG, k444><<<g, kThreads, 0, s>>>(a)));
  if (job->res < 3) {
    if (a.flags) ME_BY_SIZE(lg, (k_me_subpel<LG, true><<<g, kThreads, 0, s>>>(a)));
    else ME_BY_SIZE(lg, (k_me_subpel<LG, false><<<g, kThreads, 0, s>>>(a)));
  }
  return odhip_check_launch();
}

/* everything odhip_me_search3 refuses, the scratch apart where with_scratch is false */
int check_search3(const odhip_me_job3 *job, bool with_scratch = true) {
  const int rc = check_levels(job, with_scratch);
  if (rc) return rc;
  if (!job->levels) return check_search2(&job->base);
  const odhip_me_job *y = &job->base.luma;
  if (!y->grid || y->range < 0 || y->range > kRangeMax || y->res < 0 || y->res > 3 || y->lambda < 0
   || y->lambda > kLambdaMaxHier || job->base.lambda_subpel > kLambdaMaxHier || job->refine < 1
   || job->refine > kRefineMax) {
    return ODHIP_EINVAL;
  }
  return ODHIP_SUCCESS;
}

/* the launches of odhip_me_search3 on a checked job */
int run_search3(const odhip_me_job3 *job, int legal_lg, hipStream_t s) {
  if (!job->levels) return run_search2(&job->base, legal_lg, s);
  const odhip_me_job *y = &job->base.luma;
  const HierLayout lay = layout_of(job);
  MeArgs a = level_args(job, lay, 0);
  a.legal_lg = legal_lg;
  const size_t points = (size_t)y->npics*(a.nh + 1)*(a.nv + 1);
  ODHIP_TRY(hipMemsetAsync(y->grid, 0, points*sizeof(odhip_mv_point), s));
  if (y->cost) ODHIP_TRY(hipMemsetAsync(y->cost, 0, points*sizeof(uint32_t), s));
  int rc = build_pyramids(job, lay, s);
  if (rc) return rc;
  const int lg = y->log_size;
  const dim3 g((unsigned)(((a.nh >> lg) + 1)*((a.nv >> lg) + 1)), (unsigned)y->npics);
  for (int j = job->levels; j > 0; j--) {
    MeArgs al = level_args(job, lay, j);
    al.legal_lg = legal_lg;
    al.top = j == job->levels;
    al.range = al.top ? y->range : job->refine;
    if (j == 2) ME_BY_SIZE(lg, (launch_coarse<LG, 2>(al, g, s)));
    else ME_BY_SIZE(lg, (launch_coarse<LG, 1>(al, g, s)));
  }
  /* level 0 is stage 1 within `refine` of every slot's centre */
  a.range = job->refine;
  if (!(a.flags & ODHIP_ME_CHROMA)) ME_BY_SIZE(lg, (k_me_fullpel<LG, kNoChroma, 0><<<g, kThreads, 0, s>>>(a)));
  else if (a.cdec) ME_BY_SIZE(lg, (k_me_fullpel<LG, k420, 0><<<g, kThreads, 0, s>>>(a)));
  else ME_BY_SIZE(lg, (k_me_fullpel<LG, k444, 0><<<g, kThreads, 0, s>>>(a)));
  if (y->res < 3) {
    if (a.flags) ME_BY_SIZE(lg, (k_me_subpel<LG, true><<<g, kThreads, 0, s>>>(a)));
    else ME_BY_SIZE(lg, (k_me_subpel<LG, false><<<g, kThreads, 0, s>>>(a)));
  }
  return odhip_check_launch();
}

/* ---- variable block sizes (odhip_me_search_vbs, include/daala_hip.h): cell distortions, decisions, points ---- */

constexpr int kSizesMax = OD_MC_LOG_MVB_MAX + 1;
constexpr int kPenaltyMax = 1 << 24;

struct CellArgs {
  const uint8_t *src;
  const uint8_t *pred[kSizesMax];            /* [F] coded-size planes per size, rows w apart, 8-byte aligned */
  uint32_t *dist;                            /* [nsizes][F][nv][nh] */
  long long src_plane_stride;
  int src_stride;
  int w;
  int h;
  int pic_w;
  int pic_h;
  int nh;
  int nv;
  int npics;
  int nsizes;
};

/* Step 3: the SAD of every size's prediction against the source over every 8x8 luma cell, clipped to the picture.
   A lane owns one cell, neighbouring lanes neighbouring cells of one row of cells: a wave reads 512 bytes of a line
   at a time, 8 bytes a lane, the source once for all sizes.  The picture's edge is a byte mask (as clip_masks); a
   source line that is cut, or not 8-byte aligned, is gathered. */
__global__ __launch_bounds__(kThreads) void k_me_cell_dist(CellArgs a) {
  const int cell = (int)(blockIdx.x*kThreads + threadIdx.x);
  const int pic = blockIdx.y;
  if (cell >= a.nh*a.nv) return;
  const int cx = cell%a.nh;
  const int cy = cell/a.nh;
  const int x0 = 8*cx;
  const int y0 = 8*cy;
  const int nx = min(max(a.pic_w - x0, 0), 8);
  const int ny = min(max(a.pic_h - y0, 0), 8);
  uint32_t mask[2];
  clip_masks<2>(Clip{0, nx, 0, ny}, mask);
  uint32_t sum[kSizesMax];
#pragma unroll
  for (int si = 0; si < kSizesMax; si++) sum[si] = 0;
  const uint8_t *src = a.src + pic*a.src_plane_stride + (size_t)y0*a.src_stride + x0;
  const size_t at = ((size_t)pic*a.h + y0)*a.w + x0;
  const int rows = nx ? ny : 0;
  /* (unrolled under a predicate, so that the loads of all eight lines are in flight together) */
#pragma unroll
  for (int j = 0; j < 8; j++) {
    if (j >= rows) continue;
    const uint8_t *row = src + (size_t)j*a.src_stride;
    uint32_t s0 = 0;
    uint32_t s1 = 0;
    if (nx == 8 && !((uintptr_t)row & 7)) {
      const uint2 v = *(const uint2 *)row;
      s0 = v.x;
      s1 = v.y;
    }
    else {
      for (int b = 0; b < nx; b++) {
        if (b < 4) s0 |= (uint32_t)row[b] << 8*b;
        else s1 |= (uint32_t)row[b] << 8*(b - 4);
      }
    }
#pragma unroll
    for (int si = 0; si < kSizesMax; si++) {
      if (si < a.nsizes) {
        const uint2 v = *(const uint2 *)(a.pred[si] + at + (size_t)j*a.w);
        sum[si] = __builtin_amdgcn_sad_u8(v.x & mask[0], s0, sum[si]);
        sum[si] = __builtin_amdgcn_sad_u8(v.y & mask[1], s1, sum[si]);
      }
    }
  }
#pragma unroll
  for (int si = 0; si < kSizesMax; si++) {
    if (si < a.nsizes) a.dist[(((size_t)si*a.npics + pic)*a.nv + cy)*a.nh + cx] = sum[si];
  }
}

/* the launch of step 3 over the job's source pictures; ca holds the predictions */
void launch_cell_dist(CellArgs &ca, const odhip_me_job *y, int nsizes, uint32_t *dist, hipStream_t s) {
  ca.src = y->src;
  ca.dist = dist;
  ca.src_plane_stride = y->src_plane_stride;
  ca.src_stride = y->src_stride;
  ca.w = y->coded_w;
  ca.h = y->coded_h;
  ca.pic_w = y->pic_w;
  ca.pic_h = y->pic_h;
  ca.nh = y->coded_w >> 3;
  ca.nv = y->coded_h >> 3;
  ca.npics = y->npics;
  ca.nsizes = nsizes;
  k_me_cell_dist<<<dim3((unsigned)((ca.nh*ca.nv + kThreads - 1)/kThreads), (unsigned)y->npics), kThreads, 0, s>>>(ca);
}

struct VbsArgs {
  const uint32_t *dist;                      /* [nsizes][F][nv][nh] */
  uint32_t *bits;                            /* [F][nv/8][nh/8]: the decisions of every 64x64 cell (me_vbs.cuh) */
  const odhip_mv_point *g[kSizesMax];        /* the uniform grids, log_min first */
  const uint32_t *c[kSizesMax];              /* their costs; read only with cost */
  odhip_mv_point *grid;
  uint32_t *cost;
  int nh;
  int nv;
  int npics;
  int log_min;
  int log_max;
  int penalty;
};

/* Step 4: a wave per 64x64 cell and picture, a lane per 8x8 cell of it.  The distortions are summed up the quadtree by
   butterflies over the lane's x bits and y bits; the first lane of every cell of a size takes that cell's decision.
   Sizes above log_max always split, sizes down to log_min never: a decision reads the d arrays and nothing else. */
__global__ __launch_bounds__(64) void k_me_vbs_decide(VbsArgs a) {
  const int n64 = a.nh >> 3;
  const int cx = blockIdx.x%n64;
  const int cy = blockIdx.x/n64;
  const int pic = blockIdx.y;
  const int lx = threadIdx.x & 7;
  const int ly = threadIdx.x >> 3;
  const int nsizes = a.log_max - a.log_min + 1;
  uint32_t d[kSizesMax];
#pragma unroll
  for (int si = 0; si < kSizesMax; si++) {
    d[si] = si < nsizes ? a.dist[(((size_t)si*a.npics + pic)*a.nv + 8*cy + ly)*a.nh + 8*cx + lx] : 0;
  }
  uint32_t bits = 0;
#pragma unroll
  for (int lg = 3; lg >= 1; lg--) {
    bool split = lg > a.log_max;
    if (lg > a.log_min && lg <= a.log_max) {
      uint32_t small = 0;
      uint32_t big = 0;
#pragma unroll
      for (int si = 0; si < kSizesMax; si++) {
        if (si == lg - 1 - a.log_min) small = d[si];
        if (si == lg - a.log_min) big = d[si];
      }
#pragma unroll
      for (int b = 0; b < lg; b++) {
        small += __shfl_xor(small, 1 << b);
        big += __shfl_xor(big, 1 << b);
        small += __shfl_xor(small, 8 << b);
        big += __shfl_xor(big, 8 << b);
      }
      split = od_vbs_split(small, big, a.penalty);
    }
    if (split && !((lx | ly) & ((1 << lg) - 1))) bits |= 1u << od_vbs_bit(lg, lx, ly);
  }
  for (int s = 32; s > 0; s >>= 1) bits |= __shfl_xor(bits, s);
  if (threadIdx.x == 0) a.bits[((size_t)pic*(a.nv >> 3) + cy)*n64 + cx] = bits;
}

/* Steps 5 and 6: a lane per grid point.  Its flag follows from the decisions in closed form (od_vbs_point_valid), the
   size it takes its record from by the stateless walk over the four cells round it (od_vbs_point_size); the record is
   copied from that size's uniform grid.  Every point is written, an invalid one all zero. */
__global__ __launch_bounds__(kThreads) void k_me_vbs_grid(VbsArgs a) {
  const int t = (int)(blockIdx.x*kThreads + threadIdx.x);
  const int pic = blockIdx.y;
  const int npts = (a.nh + 1)*(a.nv + 1);
  if (t >= npts) return;
  const int x = t%(a.nh + 1);
  const int y = t/(a.nh + 1);
  const int n64 = a.nh >> 3;
  const uint32_t *mine = a.bits + (size_t)pic*(a.nv >> 3)*n64;
  auto bits = [&](int bx, int by) { return mine[by*n64 + bx]; };
  odhip_mv_point pt;
  pt.mvx = pt.mvy = 0;
  pt.valid = pt.ref = 0;
  pt.reserved = 0;
  uint32_t cost = 0;
  const size_t at = (size_t)pic*npts + t;
  if (od_vbs_point_valid(bits, x, y, a.nh, a.nv)) {
    const int s = od_vbs_point_size(bits, x, y, a.nh, a.nv);
    /* (a leaf of the pattern is never outside log_min .. log_max; the clamp keeps a read inside the arrays) */
    const int si = min(max(s, a.log_min), a.log_max) - a.log_min;
#pragma unroll
    for (int k = 0; k < kSizesMax; k++) {
      if (k == si) {
        pt = a.g[k][at];
        if (a.cost) cost = a.c[k][at];
      }
    }
    pt.valid = 1;
  }
  a.grid[at] = pt;
  if (a.cost) a.cost[at] = cost;
}

/* The private layout of a job4's scratch, from its 16-byte aligned start: per size the uniform grid, its costs and
   its prediction; the d arrays; the decisions; and one odhip_me_search3 scratch that the sizes use in turn. */
struct VbsLayout {
  size_t grid[kSizesMax];
  size_t cost[kSizesMax];
  size_t pred[kSizesMax];
  size_t dist;
  size_t bits;
  size_t hier;
  size_t hier_bytes;
  size_t bytes;
};

/* the uniform search of size lg of a job4: everything of the job3 but the size, the levels and the buffers */
odhip_me_job3 size_job(const odhip_me_job4 *job, int lg) {
  odhip_me_job3 j = job->base;
  j.base.luma.log_size = lg;
  j.levels = job->base.levels < lg + 1 ? job->base.levels : lg + 1;
  j.scratch = nullptr;
  j.scratch_bytes = 0;
  return j;
}

VbsLayout vbs_layout_of(const odhip_me_job4 *job) {
  const odhip_me_job &y = job->base.base.luma;
  VbsLayout o;
  memset(&o, 0, sizeof(o));
  size_t at = 0;
  auto take = [&](size_t n) {
    const size_t was = at;
    at += (n + 15) & ~(size_t)15;
    return was;
  };
  const size_t nh = y.coded_w >> 3;
  const size_t nv = y.coded_h >> 3;
  const size_t points = (nh + 1)*(nv + 1)*y.npics;
  const int nsizes = y.log_size - job->log_min + 1;
  for (int si = 0; si < nsizes; si++) {
    o.grid[si] = take(points*sizeof(odhip_mv_point));
    o.cost[si] = take(points*sizeof(uint32_t));
    o.pred[si] = take((size_t)y.coded_w*y.coded_h*y.npics);
    const odhip_me_job3 j = size_job(job, job->log_min + si);
    const size_t need = odhip_me_scratch_bytes(&j);
    if (need > o.hier_bytes) o.hier_bytes = need;
  }
  o.dist = take(nsizes*nh*nv*y.npics*sizeof(uint32_t));
  o.bits = take((nh >> 3)*(nv >> 3)*y.npics*sizeof(uint32_t));
  o.hier = take(o.hier_bytes);
  o.bytes = at + 16;                         /* the caller's buffer has any alignment */
  return o;
}

/* the sizes of a job4, which alone decide its scratch */
bool vbs_sizes_ok(const odhip_me_job4 *job) {
  if (!job) return false;
  const odhip_me_job &y = job->base.base.luma;
  return od_mc_size_ok(y.coded_w, y.coded_h) && y.pic_w >= 1 && y.pic_w <= y.coded_w && y.pic_h >= 1
   && y.pic_h <= y.coded_h && y.npics >= 1 && y.npics <= 65535 && y.nrefs >= 1 && y.nrefs <= 3 && y.log_size >= 0
   && y.log_size <= OD_MC_LOG_MVB_MAX && job->log_min >= 0 && job->log_min <= y.log_size && job->base.levels >= 0
   && job->base.levels <= kLevelsMax;
}

}  // namespace

extern "C" size_t odhip_me_sizeof(int what) {
  return what == 0 ? sizeof(odhip_me_job) : what == 1 ? sizeof(odhip_me_cand) : what == 2 ? sizeof(odhip_me_job2)
   : what == 4 ? sizeof(odhip_me_job3) : what == 5 ? sizeof(odhip_me_job4) : 0;
}

extern "C" int odhip_me_search2(const odhip_me_job2 *job2, odhip_stream stream) {
  const int rc = check_search2(job2);
  if (rc) return rc;
  ODHIP_CTX_OR_RETURN(ctx);
  if (ctx->fpr) return ODHIP_EIMPL;          /* 12-bit references */
  return run_search2(job2, -1, (hipStream_t)stream);
}

/* the luma SAD search: no flags, one lambda */
extern "C" int odhip_me_search(const odhip_me_job *job, odhip_stream stream) {
  if (!job) return ODHIP_EINVAL;
  odhip_me_job2 job2 = job2_of(job);
  /* an out-of-range lambda is refused as the luma job's */
  job2.lambda_subpel = job->lambda < 0 ? 0 : job->lambda > kLambdaMax ? kLambdaMax : job->lambda;
  return odhip_me_search2(&job2, stream);
}

extern "C" int odhip_me_limits(int coded_w, int coded_h, int log_size, int vx, int vy, int lim[4]) {
  if (!lim || !od_mc_size_ok(coded_w, coded_h) || log_size < 0 || log_size > OD_MC_LOG_MVB_MAX) return ODHIP_EINVAL;
  const int n[2] = {coded_w >> 3, coded_h >> 3};
  const int v[2] = {vx, vy};
  for (int i = 0; i < 2; i++) {
    if (v[i] < 0 || v[i] > n[i] || (v[i] & ((1 << log_size) - 1))) return ODHIP_EINVAL;
    /* the legal components are an interval round 0 that ends with the window at the border */
    int lo = 0;
    int hi = 0;
    while (od_me_mv_ok(v[i], 8*(lo - 1), log_size, n[i])) lo--;
    while (od_me_mv_ok(v[i], 8*(hi + 1), log_size, n[i])) hi++;
    lim[2*i] = lo;
    lim[2*i + 1] = hi;
  }
  return ODHIP_SUCCESS;
}

/* the luma SAD of every candidate, one value each; range, res and lambda are not looked at */
extern "C" int odhip_me_costs(const odhip_me_job *job, const odhip_me_cand *d_cands, long n, uint32_t *d_sad,
 odhip_stream stream) {
  if (!job) return ODHIP_EINVAL;
  const odhip_me_job2 job2 = job2_of(job);
  return me_costs(&job2, d_cands, n, 0, 1, d_sad, stream);
}

extern "C" int odhip_me_costs2(const odhip_me_job2 *job, const odhip_me_cand *d_cands, long n, int metric,
 uint32_t *d_dist, odhip_stream stream) {
  return me_costs(job, d_cands, n, metric, 3, d_dist, stream);
}

/* ---- the coarse-to-fine search (include/daala_hip.h) ---- */

extern "C" size_t odhip_me_scratch_bytes(const odhip_me_job3 *job) {
  if (!job || job->levels < 1 || job->levels > kLevelsMax) return 0;
  /* the sizes alone decide: no pointer or stride is looked at */
  const odhip_me_job &y = job->base.luma;
  if (!od_mc_size_ok(y.coded_w, y.coded_h) || y.pic_w < 1 || y.pic_w > y.coded_w || y.pic_h < 1 || y.pic_h > y.coded_h
   || y.npics < 1 || y.npics > 65535 || y.nrefs < 1 || y.nrefs > 3 || y.log_size < 0
   || y.log_size > OD_MC_LOG_MVB_MAX) {
    return 0;
  }
  return layout_of(job).bytes;
}

extern "C" int odhip_me_downsample(uint8_t *dst, int dst_stride, int64_t dst_plane_stride, const uint8_t *src,
 int src_stride, int64_t src_plane_stride, int w, int h, int nplanes, odhip_stream stream) {
  if (!dst || !src || w < 1 || h < 1 || w > 32704 || h > 32704 || nplanes < 1 || nplanes > 65535 || src_stride < w
   || dst_stride < (w + 1) >> 1 || src_plane_stride < (int64_t)src_stride*h
   || dst_plane_stride < (int64_t)dst_stride*((h + 1) >> 1)) {
    return ODHIP_EINVAL;
  }
  return halve(dst, dst_stride, dst_plane_stride, src, src_stride, src_plane_stride, w, h, nplanes,
   (hipStream_t)stream);
}

extern "C" int odhip_me_search3(const odhip_me_job3 *job, odhip_stream stream) {
  const int rc = check_search3(job);
  if (rc) return rc;
  ODHIP_CTX_OR_RETURN(ctx);
  if (ctx->fpr) return ODHIP_EIMPL;
  return run_search3(job, -1, (hipStream_t)stream);
}
/* D_level of every candidate, luma only; the search parameters but `levels` are not looked at */
extern "C" int odhip_me_costs3(const odhip_me_job3 *job, const odhip_me_cand *d_cands, long n, int level,
 uint32_t *d_sad, odhip_stream stream) {
  int rc = check_levels(job);
  if (rc) return rc;
  if (!d_cands || !d_sad || n < 0 || n > 0x7fffffffL || level < 0 || level > job->levels) return ODHIP_EINVAL;
  ODHIP_CTX_OR_RETURN(ctx);
  if (ctx->fpr) return ODHIP_EIMPL;
  HierLayout lay;
  memset(&lay, 0, sizeof(lay));
  if (job->levels) {
    lay = layout_of(job);
    rc = build_pyramids(job, lay, (hipStream_t)stream);
    if (rc) return rc;
  }
  if (!n) return ODHIP_SUCCESS;
  const MeArgs a = level_args(job, lay, level);
  k_me_level_sad<<<(unsigned)n, kThreads, 0, (hipStream_t)stream>>>(a, d_cands, job->base.luma.log_size, level,
   d_sad);
  return odhip_check_launch();
}

/* ---- variable block sizes (include/daala_hip.h) ---- */

extern "C" int odhip_me_cell_dist(const odhip_me_job *job, const uint8_t *const *pred, int nsizes, uint32_t *dist,
 odhip_stream stream) {
  const int rc = check_planes(job);
  if (rc) return rc;
  if (!pred || !dist || nsizes < 1 || nsizes > kSizesMax) return ODHIP_EINVAL;
  CellArgs ca;
  memset(&ca, 0, sizeof(ca));
  for (int si = 0; si < nsizes; si++) {
    if (!pred[si] || ((uintptr_t)pred[si] & 7)) return ODHIP_EINVAL;
    ca.pred[si] = pred[si];
  }
  ODHIP_CTX_OR_RETURN(ctx);
  if (ctx->fpr) return ODHIP_EIMPL;
  launch_cell_dist(ca, job, nsizes, dist, (hipStream_t)stream);
  return odhip_check_launch();
}

extern "C" size_t odhip_me_vbs_scratch_bytes(const odhip_me_job4 *job) {
  if (!vbs_sizes_ok(job)) return 0;
  if (job->log_min == job->base.base.luma.log_size) return odhip_me_scratch_bytes(&job->base);
  return vbs_layout_of(job).bytes;
}

extern "C" int odhip_me_search_vbs(const odhip_me_job4 *job, odhip_stream stream) {
  if (!job) return ODHIP_EINVAL;
  const odhip_me_job &y = job->base.base.luma;
  const int log_max = y.log_size;
  if (log_max < 0 || log_max > OD_MC_LOG_MVB_MAX || job->log_min < 0 || job->log_min > log_max
   || job->split_penalty < 0 || job->split_penalty > kPenaltyMax) {
    return ODHIP_EINVAL;
  }
  if (job->log_min == log_max) return odhip_me_search3(&job->base, stream);
  /* what odhip_me_search3 refuses at the largest size - the job's own levels among it - and at every size below */
  for (int lg = log_max; lg >= job->log_min; lg--) {
    odhip_me_job3 j = size_job(job, lg);
    if (lg == log_max) j.levels = job->base.levels;
    const int rc = check_search3(&j, false);
    if (rc) return rc;
  }
  const VbsLayout lay = vbs_layout_of(job);
  if (!job->base.scratch || job->base.scratch_bytes < lay.bytes) return ODHIP_EINVAL;
  ODHIP_CTX_OR_RETURN(ctx);
  if (ctx->fpr) return ODHIP_EIMPL;
  hipStream_t s = (hipStream_t)stream;
  uint8_t *base = (uint8_t *)(((uintptr_t)job->base.scratch + 15) & ~(uintptr_t)15);
  const int nsizes = log_max - job->log_min + 1;
  const int nh = y.coded_w >> 3;
  const int nv = y.coded_h >> 3;
  CellArgs ca;
  VbsArgs va;
  memset(&ca, 0, sizeof(ca));
  memset(&va, 0, sizeof(va));
  for (int si = 0; si < nsizes; si++) {
    /* steps 1 and 2: the uniform search of this size under the cells' legality, then its prediction */
    odhip_me_job3 j = size_job(job, job->log_min + si);
    j.base.luma.grid = (odhip_mv_point *)(base + lay.grid[si]);
    j.base.luma.cost = y.cost ? (uint32_t *)(base + lay.cost[si]) : nullptr;
    j.scratch = base + lay.hier;
    j.scratch_bytes = lay.hier_bytes;
    int rc = run_search3(&j, log_max, s);
    if (rc) return rc;
    odhip_mc_job mc;
    memset(&mc, 0, sizeof(mc));
    mc.coded_w = y.coded_w;
    mc.coded_h = y.coded_h;
    mc.sample = ODHIP_SAMPLE_U8;
    mc.npics = mc.nplanes = y.npics;
    mc.nrefs = y.nrefs;
    mc.grid_on_device = 1;
    mc.ref_stride = y.ref_stride;
    mc.ref_plane_stride = y.ref_plane_stride;
    mc.dst_stride = y.coded_w;
    mc.dst_plane_stride = (int64_t)y.coded_w*y.coded_h;
    for (int r = 0; r < y.nrefs; r++) mc.ref[r] = y.ref[r];
    mc.dst = base + lay.pred[si];
    mc.grid = j.base.luma.grid;
    rc = odhip_mc_predict_planes(&mc, stream);
    if (rc) return rc;
    ca.pred[si] = base + lay.pred[si];
    va.g[si] = j.base.luma.grid;
    va.c[si] = j.base.luma.cost;
  }
  va.dist = job->cell_dist ? job->cell_dist : (uint32_t *)(base + lay.dist);
  launch_cell_dist(ca, &y, nsizes, (uint32_t *)va.dist, s);
  va.bits = (uint32_t *)(base + lay.bits);
  va.grid = y.grid;
  va.cost = y.cost;
  va.nh = nh;
  va.nv = nv;
  va.npics = y.npics;
  va.log_min = job->log_min;
  va.log_max = log_max;
  va.penalty = job->split_penalty;
  k_me_vbs_decide<<<dim3((unsigned)((nh >> 3)*(nv >> 3)), (unsigned)y.npics), 64, 0, s>>>(va);
  const int npts = (nh + 1)*(nv + 1);
  k_me_vbs_grid<<<dim3((unsigned)((npts + kThreads - 1)/kThreads), (unsigned)y.npics), kThreads, 0, s>>>(va);
  return odhip_check_launch();
}
