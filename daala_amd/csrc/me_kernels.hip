/* me_kernels.hip - motion-vector grids by exhaustive block matching.

   The cost of a candidate is the reference's own block-matching cost (od_mv_est_bma_sad, src/mcenc.c:2224-2264):
   od_mc_predict1fmv8_c of one vector on the B x B block centred on a grid point (src/mcenc.c:2589-2611), then
   od_enc_sad of it against the source picture, clipped to the picture (src/mcenc.c:1615-1679).  The search over
   candidates is a fixed one (include/daala_hip.h): every full-pel offset within `range` in every slot, then
   three rounds of eight sub-pel neighbours, each won by the smallest key (cost, |mvx| + |mvy|, slot, mvy, mvx).
   A candidate is evaluated only where od_me_mv_ok (mc_walk.cuh) allows it, so every grid passes
   odhip_mc_check_grid at both decimations.  8-bit luma only.

   Three kernels, one 256-lane block per grid point and picture each:
     k_me_fullpel<LG>  stages the clamped (B + 2 range)^2 window of a slot and the source block in LDS; a lane
                       owns four neighbouring offsets of one row of the search square and slides the block over
                       them with v_qsad_pk_u16_u8 (v_sad_u8 under a byte mask where the picture edge cuts a
                       group of four columns); the packed 16-bit sums are flushed to 32 bits before they can
                       overflow; the key is reduced across the block, so the winner does not depend on the lane
     k_me_subpel<LG>   stages the winner's window, one sample wider on every side, and runs the rounds: per
                       candidate the two filter passes of mc_filter.cuh from LDS and a block-wide sum
     k_me_costs<LG>    the same candidate evaluation for listed candidates (test surface)

   odhip_me_search2 adds the two terms the reference's search has beside the luma SAD (include/daala_hip.h): the
   chroma planes in the cost (od_mv_est_bma_sad with OD_MC_USE_CHROMA: each chroma distortion >> 2) and SATD as the
   sub-pel metric (od_enc_satd).  With neither flag it launches the kernels above, so odhip_me_search is a wrapper
   over it and costs what it did.  Three more kernels serve the flags:
     k_me_fullpel2<LG, CDEC>  stage 1 with chroma: per slot the luma pass above, then one pass per chroma plane, all
                       into one LDS array of per-offset distortions (the three plane sums stay apart until the >> 2),
                       then the keys.  At CDEC = 1 an odd luma offset is a chroma half-pel: the four phase planes
                       (fx, fy in {0, 4}) of the chroma window are built once per block, slot and plane with
                       mc_hpass / mc_vpass, and a lane slides over four offsets of one parity
     k_me_subpel2<LG>  the rounds with the windows of all three planes staged; per candidate and plane the two filter
                       passes, then SAD or SATD: a lane holds one row of an 8x8 (4x4) tile of differences, the
                       horizontal butterflies run in registers, the vertical ones across 8 (4) lanes
     k_me_costs2<LG>   the same evaluation for listed candidates, the three plane distortions apart (test surface) */
#include <string.h>
#include "../../include/daala_hip.h"
#include "od_common.cuh"
#include "od_ctx.cuh"
#include "mc_walk.cuh"
#include "mc_filter.cuh"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads/64;
constexpr int kRangeMax = 32;
constexpr int kQuadsMax = (2*kRangeMax + 1 + 3)/4;   /* groups of four offsets along a row of the search square */
/* keeps the cost inside int32, for lambda and lambda_subpel alike: a tile's SATD is at most its maximal SAD (the
   8x8 Hadamard sum is <= 8 * 64 * 255, >> 3), so a plane's distortion is <= 64*64*255, chroma adds at most half of
   luma (2 * (D >> 2)): 8 * 1.5 * 64*64*255 + 2^20 * 2*(8*32 + 7) < 2^31 */
constexpr int kLambdaMax = 1 << 20;
constexpr int kMvBias = 512;                         /* |component| <= 8*kRangeMax + 7 */

struct MeArgs {
  const uint8_t *src;
  const uint8_t *ref[3];
  odhip_mv_point *grid;
  uint32_t *cost;
  long long src_plane_stride;
  long long ref_plane_stride;
  int src_stride;
  int ref_stride;
  int w;                         /* coded size */
  int h;
  int pic_w;
  int pic_h;
  int nh;
  int nv;
  int nrefs;
  int range;
  int res;
  int lambda;
};

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

/* (cost, |mvx| + |mvy|, slot, mvy, mvx) as one integer whose order is the lexicographic one */
__device__ inline unsigned long long me_key(int cost, int slot, int mvx, int mvy) {
  return (unsigned long long)(unsigned)cost << 32 | (unsigned long long)(abs(mvx) + abs(mvy)) << 22
   | (unsigned long long)slot << 20 | (unsigned long long)(mvy + kMvBias) << 10 | (unsigned long long)(mvx + kMvBias);
}
__device__ inline int key_mvx(unsigned long long k) { return (int)(k & 1023) - kMvBias; }
__device__ inline int key_mvy(unsigned long long k) { return (int)(k >> 10 & 1023) - kMvBias; }
__device__ inline int key_slot(unsigned long long k) { return (int)(k >> 20 & 3); }

__device__ inline int me_cost(int sad, int lambda, int mvx, int mvy) {
  return 8*sad + lambda*(abs(mvx) + abs(mvy));
}

__device__ inline void write_point(const MeArgs &a, int pic, int vx, int vy, unsigned long long key) {
  const size_t at = ((size_t)pic*(a.nv + 1) + vy)*(a.nh + 1) + vx;
  odhip_mv_point pt;
  pt.mvx = key_mvx(key);
  pt.mvy = key_mvy(key);
  pt.valid = 1;
  pt.ref = (uint8_t)key_slot(key);
  pt.reserved = 0;
  a.grid[at] = pt;
  if (a.cost) a.cost[at] = (uint32_t)(key >> 32);
}

/* the source block as rows of B bytes; coordinates outside the picture are clamped (the clip rectangle keeps
   those samples out of every sum) */
template <int B>
__device__ inline void stage_block(uint8_t *blk, const uint8_t *src, int stride, int bx, int by, int pic_w,
 int pic_h) {
  for (int e = threadIdx.x; e < B*B; e += kThreads) {
    const int x = min(max(bx + e%B, 0), pic_w - 1);
    const int y = min(max(by + e/B, 0), pic_h - 1);
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

template <int LG>
__global__ __launch_bounds__(kThreads) void k_me_fullpel(MeArgs a) {
  constexpr int B = 8 << LG;
  constexpr int G = B/4;                     /* groups of four columns across the block */
  constexpr int WD = G + kQuadsMax;          /* the widest window row, in dwords */
  constexpr int WR = B + 2*kRangeMax;
  __shared__ uint32_t win[WR*WD];
  __shared__ uint32_t blk[B*G];
  __shared__ uint8_t okx[4*kQuadsMax];
  __shared__ uint8_t oky[2*kRangeMax + 1];
  __shared__ unsigned long long red[kWaves];
  const int npx = (a.nh >> LG) + 1;
  const int vx = (int)(blockIdx.x%npx) << LG;
  const int vy = (int)(blockIdx.x/npx) << LG;
  const int pic = blockIdx.y;
  const int bx = 8*vx - B/2;
  const int by = 8*vy - B/2;
  const int r = a.range;
  const int side = 2*r + 1;
  const int nq = (side + 3) >> 2;
  const int wd = G + nq;
  const Clip c = clip_of(bx, by, B, a.pic_w, a.pic_h);
  stage_block<B>((uint8_t *)blk, a.src + pic*a.src_plane_stride, a.src_stride, bx, by, a.pic_w, a.pic_h);
  for (int e = threadIdx.x; e < 4*nq; e += kThreads) okx[e] = e < side && od_me_mv_ok(vx, 8*(e - r), LG, a.nh);
  for (int e = threadIdx.x; e < side; e += kThreads) oky[e] = od_me_mv_ok(vy, 8*(e - r), LG, a.nv);
  /* which bytes of each group of four columns are inside the picture */
  uint32_t mask[G];
#pragma unroll
  for (int g = 0; g < G; g++) {
    const int lo = min(max(c.x0 - 4*g, 0), 4);
    const int hi = min(max(c.x1 - 4*g, 0), 4);
    mask[g] = hi <= lo ? 0u : (hi == 4 ? ~0u : (1u << 8*hi) - 1) & ~((1u << 8*lo) - 1);
  }
  unsigned long long best = ~0ull;
  for (int slot = 0; slot < a.nrefs; slot++) {
    const uint8_t *ref = a.ref[slot] + pic*a.ref_plane_stride;
    __syncthreads();                         /* the previous slot's lanes have read the window */
    for (int e = threadIdx.x; e < (B + 2*r)*wd; e += kThreads) {
      const int y = min(max(by - r + e/wd, 0), a.h - 1);
      const int x0 = bx - r + 4*(e%wd);
      const uint8_t *row = ref + (size_t)y*a.ref_stride;
      uint32_t v = 0;
#pragma unroll
      for (int b = 0; b < 4; b++) v |= (uint32_t)row[min(max(x0 + b, 0), a.w - 1)] << 8*b;
      win[e] = v;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < side*nq; t += kThreads) {
      const int dyi = t/nq;
      const int q = t%nq;
      uint32_t sad[4] = {0, 0, 0, 0};
      unsigned long long acc = 0;            /* four packed 16-bit sums */
      int pending = 0;                       /* quad SADs in acc: each adds at most 4*255 */
      for (int j = c.y0; j < c.y1; j++) {
        const uint32_t *wrow = &win[(j + dyi)*wd + q];
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
        if (pending > 64 - G) {              /* 64 quad SADs are the most 16 bits hold */
#pragma unroll
          for (int k = 0; k < 4; k++) sad[k] += (uint32_t)(acc >> 16*k) & 0xffff;
          acc = 0;
          pending = 0;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; k++) sad[k] += (uint32_t)(acc >> 16*k) & 0xffff;
      const int mvy = 8*(dyi - r);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int mvx = 8*(4*q + k - r);
        if (!okx[4*q + k] || !oky[dyi]) continue;
        const unsigned long long key = me_key(me_cost((int)sad[k], a.lambda, mvx, mvy), slot, mvx, mvy);
        best = key < best ? key : best;
      }
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long other = __shfl_xor(best, d);
    best = other < best ? other : best;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kWaves; i++) best = red[i] < best ? red[i] : best;
    write_point(a, pic, vx, vy, best);
  }
}

/* LDS of one candidate evaluation: the winner's window (one sample wider on every side than one vector's
   B + 5), the first filter pass, the source block */
template <int B>
struct CandLds {
  static constexpr int WP = B + kApron + 1;
  uint8_t win[WP*WP];
  int16_t mid[(B + kApron)*B];
  uint8_t blk[B*B];
  int red[kWaves];
};

/* SAD of the prediction at phases (fx, fy) from the window at offset (ox, oy) against the source block inside
   the clip rectangle; every lane of the block calls it and gets the sum */
template <int B>
__device__ inline int cand_sad(CandLds<B> &l, int ox, int oy, int fx, int fy, Clip c) {
  constexpr int WP = CandLds<B>::WP;
  if (fx | fy) {
    for (int e = threadIdx.x; e < (B + kApron)*B; e += kThreads) {
      l.mid[e] = (int16_t)mc_hpass<uint8_t>(&l.win[(oy + e/B)*WP + ox + e%B], fx);
    }
  }
  __syncthreads();
  int acc = 0;
  for (int e = threadIdx.x; e < B*B; e += kThreads) {
    const int i = e%B;
    const int j = e/B;
    if (i < c.x0 || i >= c.x1 || j < c.y0 || j >= c.y1) continue;
    const int p = (fx | fy) ? (int)mc_vpass<uint8_t>(&l.mid[e], B, fy) : (int)l.win[(oy + j + kTop)*WP + ox + i + kTop];
    acc += abs(p - (int)l.blk[e]);
  }
  for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
  if ((threadIdx.x & 63) == 0) l.red[threadIdx.x >> 6] = acc;
  __syncthreads();
  int sum = 0;
  for (int i = 0; i < kWaves; i++) sum += l.red[i];
  __syncthreads();                           /* red and mid are free again */
  return sum;
}

template <int LG>
__global__ __launch_bounds__(kThreads) void k_me_subpel(MeArgs a) {
  constexpr int B = 8 << LG;
  __shared__ CandLds<B> l;
  const int npx = (a.nh >> LG) + 1;
  const int vx = (int)(blockIdx.x%npx) << LG;
  const int vy = (int)(blockIdx.x/npx) << LG;
  const int pic = blockIdx.y;
  const int bx = 8*vx - B/2;
  const int by = 8*vy - B/2;
  const odhip_mv_point pt = a.grid[((size_t)pic*(a.nv + 1) + vy)*(a.nh + 1) + vx];
  const int slot = min((int)pt.ref, a.nrefs - 1);
  /* the full-pel winner, a multiple of 8; every candidate of the rounds is within 7 of it */
  const int fpx = pt.mvx >> 3;
  const int fpy = pt.mvy >> 3;
  const Clip c = clip_of(bx, by, B, a.pic_w, a.pic_h);
  stage_block<B>(l.blk, a.src + pic*a.src_plane_stride, a.src_stride, bx, by, a.pic_w, a.pic_h);
  stage_window(l.win, CandLds<B>::WP, a.ref[slot] + pic*a.ref_plane_stride, a.ref_stride, bx + fpx - kTop - 1,
   by + fpy - kTop - 1, a.w, a.h);
  __syncthreads();
  auto eval = [&](int mvx, int mvy) {
    const int sad = cand_sad<B>(l, (mvx >> 3) - fpx + 1, (mvy >> 3) - fpy + 1, mvx & 7, mvy & 7, c);
    return me_key(me_cost(sad, a.lambda, mvx, mvy), slot, mvx, mvy);
  };
  unsigned long long best = eval(8*fpx, 8*fpy);
  for (int step = 4; step >= 1 << a.res; step >>= 1) {
    const int cx = key_mvx(best);
    const int cy = key_mvy(best);
    for (int n = 0; n < 9; n++) {
      const int mvx = cx + (n%3 - 1)*step;
      const int mvy = cy + (n/3 - 1)*step;
      if (n == 4 || !od_me_mv_ok(vx, mvx, LG, a.nh) || !od_me_mv_ok(vy, mvy, LG, a.nv)) continue;
      const unsigned long long key = eval(mvx, mvy);
      best = key < best ? key : best;
    }
  }
  if (threadIdx.x == 0) write_point(a, pic, vx, vy, best);
}

template <int LG>
__global__ __launch_bounds__(kThreads) void k_me_costs(MeArgs a, int npics, const odhip_me_cand *cands,
 uint32_t *sad) {
  constexpr int B = 8 << LG;
  __shared__ CandLds<B> l;
  const odhip_me_cand cd = cands[blockIdx.x];
  if (cd.pic < 0 || cd.pic >= npics || cd.vx < 0 || cd.vx > a.nh || cd.vy < 0 || cd.vy > a.nv || cd.slot < 0
   || cd.slot >= a.nrefs || abs(cd.mvx) >= 1 << 20 || abs(cd.mvy) >= 1 << 20) {
    if (threadIdx.x == 0) sad[blockIdx.x] = ~0u;
    return;
  }
  const int bx = 8*cd.vx - B/2;
  const int by = 8*cd.vy - B/2;
  const Clip c = clip_of(bx, by, B, a.pic_w, a.pic_h);
  stage_block<B>(l.blk, a.src + cd.pic*a.src_plane_stride, a.src_stride, bx, by, a.pic_w, a.pic_h);
  stage_window(l.win, CandLds<B>::WP, a.ref[cd.slot] + cd.pic*a.ref_plane_stride, a.ref_stride,
   bx + (cd.mvx >> 3) - kTop, by + (cd.mvy >> 3) - kTop, a.w, a.h);
  __syncthreads();
  const int sum = cand_sad<B>(l, 0, 0, cd.mvx & 7, cd.mvy & 7, c);
  if (threadIdx.x == 0) sad[blockIdx.x] = (uint32_t)sum;
}

/* ---- chroma in the cost, SATD as the sub-pel metric (odhip_me_search2) ---- */

struct MeArgs2 {
  MeArgs y;                      /* luma; y.lambda is stage 1's */
  const uint8_t *csrc;           /* [2F] chroma pictures, all Cb then all Cr */
  const uint8_t *cref[3];
  long long csrc_plane_stride;
  long long cref_plane_stride;
  int csrc_stride;
  int cref_stride;
  int npics;
  int flags;
  int cdec;
  int lambda_subpel;
};

__device__ inline int plane_sz(int n, int d) { return (n + (1 << d) - 1) >> d; }

/* picture, reference plane and geometry of plane pl (0 luma, 1 Cb, 2 Cr) of picture pic in slot */
struct PlaneOf {
  const uint8_t *src;
  const uint8_t *ref;
  int src_stride, ref_stride;
  int w, h, pic_w, pic_h;        /* plane and picture size at the plane's decimation */
  int d;
};

__device__ inline PlaneOf plane_of(const MeArgs2 &a, int pl, int pic, int slot) {
  PlaneOf o;
  if (!pl) {
    o.src = a.y.src + pic*a.y.src_plane_stride;
    o.ref = a.y.ref[slot] + pic*a.y.ref_plane_stride;
    o.src_stride = a.y.src_stride;
    o.ref_stride = a.y.ref_stride;
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
  o.w = a.y.w >> o.d;
  o.h = a.y.h >> o.d;
  o.pic_w = plane_sz(a.y.pic_w, o.d);
  o.pic_h = plane_sz(a.y.pic_h, o.d);
  return o;
}

/* stage_block for a block size known at run time */
__device__ inline void stage_block_n(uint8_t *blk, int n, const uint8_t *src, int stride, int bx, int by, int pic_w,
 int pic_h) {
  for (int e = threadIdx.x; e < n*n; e += kThreads) {
    const int x = min(max(bx + e%n, 0), pic_w - 1);
    const int y = min(max(by + e/n, 0), pic_h - 1);
    blk[e] = src[(size_t)y*stride + x];
  }
}

/* One row of the search square slid over a block: the SADs of four neighbouring window offsets (dwords q .. of the
   window rows from row0 on, wd dwords apart) against the block's rows y0 .. y1 of G dwords, under the byte masks of
   the clip rectangle.  The loop of k_me_fullpel. */
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

/* LDS plan of k_me_fullpel2 */
template <int LG, int CDEC>
struct Full2 {
  static constexpr int B = 8 << LG;
  static constexpr int G = B/4;
  static constexpr int BC = B >> CDEC;
  static constexpr int GC = BC/4;
  static constexpr int kSide = 2*kRangeMax + 1;
  static constexpr int WD = G + kQuadsMax;
  static constexpr int WR = B + 2*kRangeMax;
  /* CDEC = 1: chroma integer offsets -kRcMax .. kRangeMax/2, a phase plane of P rows of PD dwords, built from a raw
     window of R x R samples */
  static constexpr int kRcMax = (kRangeMax + 1)/2;
  static constexpr int kNcoMax = kRangeMax/2 + kRcMax + 1;
  static constexpr int P = BC + kNcoMax - 1;
  static constexpr int PD = GC + (kNcoMax + 3)/4;
  static constexpr int R = P + kApron;
  static constexpr int kWinLuma = WR*WD;
  static constexpr int kWinPhase = CDEC ? 4*P*PD : 0;
  static constexpr int kWin = kWinLuma > kWinPhase ? kWinLuma : kWinPhase;   /* dwords */
  static constexpr int kRaw = CDEC ? (R*R + 3)/4 : 1;                        /* dwords */
  static constexpr int kMid = CDEC ? R*P : 2;                                /* int16 */
};

template <int LG, int CDEC>
__global__ __launch_bounds__(kThreads) void k_me_fullpel2(MeArgs2 a2) {
  typedef Full2<LG, CDEC> L;
  constexpr int B = L::B, G = L::G, BC = L::BC, GC = L::GC;
  __shared__ uint32_t win[L::kWin];
  __shared__ uint32_t blk[B*G];
  __shared__ uint32_t cblk[2][BC*GC];
  __shared__ uint32_t dist[L::kSide*4*kQuadsMax];
  __shared__ uint32_t raw[L::kRaw];
  __shared__ int16_t mid[L::kMid];
  __shared__ uint8_t okx[4*kQuadsMax];
  __shared__ uint8_t oky[2*kRangeMax + 1];
  __shared__ unsigned long long red[kWaves];
  const MeArgs &a = a2.y;
  const int npx = (a.nh >> LG) + 1;
  const int vx = (int)(blockIdx.x%npx) << LG;
  const int vy = (int)(blockIdx.x/npx) << LG;
  const int pic = blockIdx.y;
  const int bx = 8*vx - B/2;
  const int by = 8*vy - B/2;
  const int cbx = bx >> CDEC;
  const int cby = by >> CDEC;
  const int r = a.range;
  const int side = 2*r + 1;
  const int nq = (side + 3) >> 2;
  const int wd = G + nq;
  const int dp = 4*nq;                       /* row pitch of dist */
  const Clip c = clip_of(bx, by, B, a.pic_w, a.pic_h);
  const Clip cc = clip_of(cbx, cby, BC, plane_sz(a.pic_w, CDEC), plane_sz(a.pic_h, CDEC));
  stage_block<B>((uint8_t *)blk, a.src + pic*a.src_plane_stride, a.src_stride, bx, by, a.pic_w, a.pic_h);
  for (int pi = 0; pi < 2; pi++) {
    const PlaneOf o = plane_of(a2, 1 + pi, pic, 0);
    stage_block_n((uint8_t *)cblk[pi], BC, o.src, o.src_stride, cbx, cby, o.pic_w, o.pic_h);
  }
  for (int e = threadIdx.x; e < 4*nq; e += kThreads) okx[e] = e < side && od_me_mv_ok(vx, 8*(e - r), LG, a.nh);
  for (int e = threadIdx.x; e < side; e += kThreads) oky[e] = od_me_mv_ok(vy, 8*(e - r), LG, a.nv);
  unsigned long long best = ~0ull;
  for (int slot = 0; slot < a.nrefs; slot++) {
    __syncthreads();                         /* the previous slot's lanes have read dist and the window */
    stage_slide_window(win, B, r, wd, a.ref[slot] + pic*a.ref_plane_stride, a.ref_stride, bx, by, a.w, a.h);
    __syncthreads();
    {
      uint32_t mask[G];
      clip_masks<G>(c, mask);
      for (int t = threadIdx.x; t < side*nq; t += kThreads) {
        const int dyi = t/nq;
        const int q = t%nq;
        uint32_t sad[4];
        slide_sad<G>(win, wd, dyi, q, blk, mask, c.y0, c.y1, sad);
#pragma unroll
        for (int k = 0; k < 4; k++) dist[dyi*dp + 4*q + k] = sad[k];
      }
    }
    uint32_t cmask[GC];
    clip_masks<GC>(cc, cmask);
    for (int pi = 0; pi < 2; pi++) {
      const PlaneOf o = plane_of(a2, 1 + pi, pic, slot);
      __syncthreads();                       /* the pass before has read the window */
      if constexpr (CDEC == 0) {
        /* chroma slides like luma; a lane owns the offsets it owned in the luma pass */
        stage_slide_window(win, BC, r, wd, o.ref, o.ref_stride, cbx, cby, o.w, o.h);
        __syncthreads();
        for (int t = threadIdx.x; t < side*nq; t += kThreads) {
          const int dyi = t/nq;
          const int q = t%nq;
          uint32_t sad[4];
          slide_sad<GC>(win, wd, dyi, q, cblk[pi], cmask, cc.y0, cc.y1, sad);
#pragma unroll
          for (int k = 0; k < 4; k++) dist[dyi*dp + 4*q + k] += sad[k] >> 2;
        }
      }
      else {
        /* luma offset dx is the chroma vector 4 dx eighth-pels: sample offset dx >> 1 at phase 4 (dx & 1) */
        const int rc = (r + 1) >> 1;
        const int nco = (r >> 1) + rc + 1;   /* chroma sample offsets -rc .. r >> 1 */
        const int nqc = (nco + 3) >> 2;
        const int p = BC + nco - 1;          /* rows and columns of a phase plane */
        const int pd = GC + nqc;
        const int rs = p + kApron;
        uint8_t *rawb = (uint8_t *)raw;
        stage_window(rawb, rs, o.ref, o.ref_stride, cbx - rc - kTop, cby - rc - kTop, o.w, o.h);
        __syncthreads();
        for (int px = 0; px < 2; px++) {
          /* both passes for every phase, as od_mc_predict1fmv8_c runs them, the first kept in int16 */
          for (int e = threadIdx.x; e < rs*p; e += kThreads) {
            mid[e] = (int16_t)mc_hpass<uint8_t>(&rawb[(e/p)*rs + e%p], 4*px);
          }
          __syncthreads();
          for (int py = 0; py < 2; py++) {
            uint8_t *plane = (uint8_t *)&win[(px + 2*py)*p*pd];
            for (int e = threadIdx.x; e < p*4*pd; e += kThreads) {
              const int x = e%(4*pd);
              const int y = e/(4*pd);
              plane[e] = x < p ? mc_vpass<uint8_t>(&mid[y*p + x], p, 4*py) : (uint8_t)0;
            }
          }
          __syncthreads();                   /* mid is free again; after px = 1 the planes are complete */
        }
        /* a lane slides over four offsets of one parity: neighbours in that parity's plane */
        for (int t = threadIdx.x; t < side*2*nqc; t += kThreads) {
          const int dyi = t/(2*nqc);
          const int px = t%(2*nqc)/nqc;
          const int q = t%nqc;
          const int dy = dyi - r;
          uint32_t sad[4];
          slide_sad<GC>(&win[(px + 2*(dy & 1))*p*pd], pd, (dy >> 1) + rc, q, cblk[pi], cmask, cc.y0, cc.y1, sad);
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const int oi = 4*q + k;
            const int dx = 2*(oi - rc) + px;
            if (oi < nco && abs(dx) <= r) dist[dyi*dp + dx + r] += sad[k] >> 2;
          }
        }
      }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < side*side; t += kThreads) {
      const int dyi = t/side;
      const int dxi = t%side;
      if (!okx[dxi] || !oky[dyi]) continue;
      const int mvx = 8*(dxi - r);
      const int mvy = 8*(dyi - r);
      const unsigned long long key = me_key(me_cost((int)dist[dyi*dp + dxi], a.lambda, mvx, mvy), slot, mvx, mvy);
      best = key < best ? key : best;
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long other = __shfl_xor(best, d);
    best = other < best ? other : best;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kWaves; i++) best = red[i] < best ? red[i] : best;
    write_point(a, pic, vx, vy, best);
  }
}

/* LDS of one candidate evaluation over three planes: per plane the window (one sample wider on every side than one
   vector's n + 5, rows WP apart whatever the plane's n) and the source block (rows n apart), one first filter pass */
template <int B>
struct Cand2Lds {
  static constexpr int WP = B + kApron + 1;
  uint8_t win[3][WP*WP];
  int16_t mid[(B + kApron)*B];
  uint8_t blk[3][B*B];
  int red[kWaves];
};

/* Distortion of plane pl's prediction (block size n, phases (fx, fy), window offset (ox, oy)) against its source
   block inside the clip rectangle: SAD, or with satd od_enc_satd's dispatch on the clipped size - a w x w square
   of 4 takes the 4x4 Hadamard, (sum + 2) >> 2; of 8 .. 64 the 8x8 one per tile, (sum + 4) >> 3 per tile; anything
   else the SAD.  Every lane of the block calls it and gets the sum. */
template <int B>
__device__ inline int plane_dist(Cand2Lds<B> &l, int pl, int n, int ox, int oy, int fx, int fy, Clip c, bool satd) {
  constexpr int WP = Cand2Lds<B>::WP;
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
  if (satd && cw == ch && (cw == 4 || (cw >= 8 && !(cw & (cw - 1))))) {
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

template <int LG>
__global__ __launch_bounds__(kThreads) void k_me_subpel2(MeArgs2 a2) {
  constexpr int B = 8 << LG;
  constexpr int WP = Cand2Lds<B>::WP;
  __shared__ Cand2Lds<B> l;
  const MeArgs &a = a2.y;
  const int npx = (a.nh >> LG) + 1;
  const int vx = (int)(blockIdx.x%npx) << LG;
  const int vy = (int)(blockIdx.x/npx) << LG;
  const int pic = blockIdx.y;
  const int bx = 8*vx - B/2;
  const int by = 8*vy - B/2;
  const odhip_mv_point pt = a.grid[((size_t)pic*(a.nv + 1) + vy)*(a.nh + 1) + vx];
  const int slot = min((int)pt.ref, a.nrefs - 1);
  const int nplanes = a2.flags & ODHIP_ME_CHROMA ? 3 : 1;
  const bool satd = (a2.flags & ODHIP_ME_SATD) != 0;
  /* the full-pel winner at each plane's decimation: every candidate of the rounds is within 7 eighth-pels of it,
     scaled to dec = 1 within 4 - one sample either way */
  int fpx[3], fpy[3];
  Clip c[3];
  /* (unrolled, so that the per-plane values stay in registers) */
#pragma unroll
  for (int pl = 0; pl < 3; pl++) {
    if (pl >= nplanes) continue;
    const PlaneOf o = plane_of(a2, pl, pic, slot);
    const int n = B >> o.d;
    fpx[pl] = od_mc_scale_mv(pt.mvx, o.d) >> 3;
    fpy[pl] = od_mc_scale_mv(pt.mvy, o.d) >> 3;
    c[pl] = clip_of(bx >> o.d, by >> o.d, n, o.pic_w, o.pic_h);
    stage_block_n(l.blk[pl], n, o.src, o.src_stride, bx >> o.d, by >> o.d, o.pic_w, o.pic_h);
    stage_window(l.win[pl], WP, o.ref, o.ref_stride, (bx >> o.d) + fpx[pl] - kTop - 1,
     (by >> o.d) + fpy[pl] - kTop - 1, o.w, o.h);
  }
  __syncthreads();
  auto eval = [&](int mvx, int mvy) {
    int dist = 0;
#pragma unroll
    for (int pl = 0; pl < 3; pl++) {
      if (pl >= nplanes) continue;
      const int d = pl ? a2.cdec : 0;
      const int sx = od_mc_scale_mv(mvx, d);
      const int sy = od_mc_scale_mv(mvy, d);
      const int v = plane_dist<B>(l, pl, B >> d, (sx >> 3) - fpx[pl] + 1, (sy >> 3) - fpy[pl] + 1, sx & 7, sy & 7,
       c[pl], satd);
      dist += pl ? v >> 2 : v;
    }
    return me_key(me_cost(dist, a2.lambda_subpel, mvx, mvy), slot, mvx, mvy);
  };
  unsigned long long best = eval(pt.mvx, pt.mvy);
  for (int step = 4; step >= 1 << a.res; step >>= 1) {
    const int cx = key_mvx(best);
    const int cy = key_mvy(best);
    for (int n = 0; n < 9; n++) {
      const int mvx = cx + (n%3 - 1)*step;
      const int mvy = cy + (n/3 - 1)*step;
      if (n == 4 || !od_me_mv_ok(vx, mvx, LG, a.nh) || !od_me_mv_ok(vy, mvy, LG, a.nv)) continue;
      const unsigned long long key = eval(mvx, mvy);
      best = key < best ? key : best;
    }
  }
  if (threadIdx.x == 0) write_point(a, pic, vx, vy, best);
}

template <int LG>
__global__ __launch_bounds__(kThreads) void k_me_costs2(MeArgs2 a2, const odhip_me_cand *cands, int satd,
 uint32_t *out) {
  constexpr int B = 8 << LG;
  constexpr int WP = Cand2Lds<B>::WP;
  __shared__ Cand2Lds<B> l;
  const MeArgs &a = a2.y;
  const odhip_me_cand cd = cands[blockIdx.x];
  uint32_t *res = out + 3*(size_t)blockIdx.x;
  if (cd.pic < 0 || cd.pic >= a2.npics || cd.vx < 0 || cd.vx > a.nh || cd.vy < 0 || cd.vy > a.nv || cd.slot < 0
   || cd.slot >= a.nrefs || abs(cd.mvx) >= 1 << 20 || abs(cd.mvy) >= 1 << 20) {
    if (threadIdx.x < 3) res[threadIdx.x] = ~0u;
    return;
  }
  const int bx = 8*cd.vx - B/2;
  const int by = 8*cd.vy - B/2;
  const int nplanes = a2.flags & ODHIP_ME_CHROMA ? 3 : 1;
  for (int pl = 0; pl < 3; pl++) {
    if (pl >= nplanes) {
      if (threadIdx.x == 0) res[pl] = 0;
      continue;
    }
    const PlaneOf o = plane_of(a2, pl, cd.pic, cd.slot);
    const int n = B >> o.d;
    const int sx = od_mc_scale_mv(cd.mvx, o.d);
    const int sy = od_mc_scale_mv(cd.mvy, o.d);
    const Clip c = clip_of(bx >> o.d, by >> o.d, n, o.pic_w, o.pic_h);
    stage_block_n(l.blk[pl], n, o.src, o.src_stride, bx >> o.d, by >> o.d, o.pic_w, o.pic_h);
    stage_window(l.win[pl], WP, o.ref, o.ref_stride, (bx >> o.d) + (sx >> 3) - kTop, (by >> o.d) + (sy >> 3) - kTop,
     o.w, o.h);
    __syncthreads();
    const int sum = plane_dist<B>(l, pl, n, 0, 0, sx & 7, sy & 7, c, satd != 0);
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

MeArgs args_of(const odhip_me_job *job) {
  MeArgs a;
  a.src = job->src;
  for (int r = 0; r < 3; r++) a.ref[r] = r < job->nrefs ? job->ref[r] : nullptr;
  a.grid = job->grid;
  a.cost = job->cost;
  a.src_plane_stride = job->src_plane_stride;
  a.ref_plane_stride = job->ref_plane_stride;
  a.src_stride = job->src_stride;
  a.ref_stride = job->ref_stride;
  a.w = job->coded_w;
  a.h = job->coded_h;
  a.pic_w = job->pic_w;
  a.pic_h = job->pic_h;
  a.nh = job->coded_w >> 3;
  a.nv = job->coded_h >> 3;
  a.nrefs = job->nrefs;
  a.range = job->range;
  a.res = job->res;
  a.lambda = job->lambda;
  return a;
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

MeArgs2 args2_of(const odhip_me_job2 *job) {
  MeArgs2 a;
  a.y = args_of(&job->luma);
  const bool chroma = (job->flags & ODHIP_ME_CHROMA) != 0;
  a.csrc = chroma ? job->csrc : nullptr;
  for (int r = 0; r < 3; r++) a.cref[r] = chroma && r < job->luma.nrefs ? job->cref[r] : nullptr;
  a.csrc_plane_stride = job->csrc_plane_stride;
  a.cref_plane_stride = job->cref_plane_stride;
  a.csrc_stride = job->csrc_stride;
  a.cref_stride = job->cref_stride;
  a.npics = job->luma.npics;
  a.flags = job->flags;
  a.cdec = job->cdec;
  a.lambda_subpel = job->lambda_subpel;
  return a;
}

}  // namespace

extern "C" size_t odhip_me_sizeof(int what) {
  return what == 0 ? sizeof(odhip_me_job) : what == 1 ? sizeof(odhip_me_cand) : what == 2 ? sizeof(odhip_me_job2) : 0;
}

extern "C" int odhip_me_search2(const odhip_me_job2 *job2, odhip_stream stream) {
  int rc = check_job2(job2);
  if (rc) return rc;
  const odhip_me_job *job = &job2->luma;
  if (!job->grid || job->range < 0 || job->range > kRangeMax || job->res < 0 || job->res > 3 || job->lambda < 0
   || job->lambda > kLambdaMax) {
    return ODHIP_EINVAL;
  }
  ODHIP_CTX_OR_RETURN(ctx);
  if (ctx->fpr) return ODHIP_EIMPL;          /* 12-bit references */
  hipStream_t s = (hipStream_t)stream;
  const MeArgs2 a2 = args2_of(job2);
  const MeArgs &a = a2.y;
  const size_t points = (size_t)job->npics*(a.nh + 1)*(a.nv + 1);
  /* the points between the searched ones are all zero */
  ODHIP_TRY(hipMemsetAsync(job->grid, 0, points*sizeof(odhip_mv_point), s));
  if (job->cost) ODHIP_TRY(hipMemsetAsync(job->cost, 0, points*sizeof(uint32_t), s));
  const int lg = job->log_size;
  const dim3 g((unsigned)(((a.nh >> lg) + 1)*((a.nv >> lg) + 1)), (unsigned)job->npics);
  /* stage 1 is a SAD search under either metric: only chroma takes it off the luma kernel */
  if (!(job2->flags & ODHIP_ME_CHROMA)) ME_BY_SIZE(lg, (k_me_fullpel<LG><<<g, kThreads, 0, s>>>(a)));
  else if (job2->cdec) ME_BY_SIZE(lg, (k_me_fullpel2<LG, 1><<<g, kThreads, 0, s>>>(a2)));
  else ME_BY_SIZE(lg, (k_me_fullpel2<LG, 0><<<g, kThreads, 0, s>>>(a2)));
  if (job->res < 3) {
    if (job2->flags) ME_BY_SIZE(lg, (k_me_subpel2<LG><<<g, kThreads, 0, s>>>(a2)));
    else {
      MeArgs b = a;
      b.lambda = job2->lambda_subpel;
      ME_BY_SIZE(lg, (k_me_subpel<LG><<<g, kThreads, 0, s>>>(b)));
    }
  }
  return odhip_check_launch();
}

/* the luma SAD search: no flags, one lambda - the same kernels with the same arguments as before there was a job2 */
extern "C" int odhip_me_search(const odhip_me_job *job, odhip_stream stream) {
  if (!job) return ODHIP_EINVAL;
  odhip_me_job2 job2;
  memset(&job2, 0, sizeof(job2));
  job2.luma = *job;
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

extern "C" int odhip_me_costs(const odhip_me_job *job, const odhip_me_cand *d_cands, long n, uint32_t *d_sad,
 odhip_stream stream) {
  const int rc = check_planes(job);
  if (rc) return rc;
  if (!d_cands || !d_sad || n < 0 || n > 0x7fffffffL) return ODHIP_EINVAL;
  ODHIP_CTX_OR_RETURN(ctx);
  if (ctx->fpr) return ODHIP_EIMPL;
  if (!n) return ODHIP_SUCCESS;
  const MeArgs a = args_of(job);
  ME_BY_SIZE(job->log_size,
   (k_me_costs<LG><<<(unsigned)n, kThreads, 0, (hipStream_t)stream>>>(a, job->npics, d_cands, d_sad)));
  return odhip_check_launch();
}

extern "C" int odhip_me_costs2(const odhip_me_job2 *job, const odhip_me_cand *d_cands, long n, int metric,
 uint32_t *d_dist, odhip_stream stream) {
  const int rc = check_job2(job);
  if (rc) return rc;
  if (!d_cands || !d_dist || n < 0 || n > 0x7fffffffL || metric < 0 || metric > 1) return ODHIP_EINVAL;
  ODHIP_CTX_OR_RETURN(ctx);
  if (ctx->fpr) return ODHIP_EIMPL;
  if (!n) return ODHIP_SUCCESS;
  const MeArgs2 a2 = args2_of(job);
  ME_BY_SIZE(job->luma.log_size,
   (k_me_costs2<LG><<<(unsigned)n, kThreads, 0, (hipStream_t)stream>>>(a2, d_cands, metric, d_dist)));
  return odhip_check_launch();
}
