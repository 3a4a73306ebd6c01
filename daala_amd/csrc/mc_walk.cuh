/* mc_walk.cuh - the leaf walk of a motion-vector grid, shared by the classification kernel and the host-side
   validation (mc_kernels.hip), and the legal range of a vector, shared by that validation and the motion search
   (me_kernels.hip).

   The grid has a point every 8 luma pixels; a 64x64 cell splits into quadrants while the point at its centre is
   valid (od_state_pred_block, src/state.c:673-722).  The walk has no state: the leaf that covers an 8x8 cell is
   found by testing at most three centre points from the top size down, so one lane per cell classifies a whole
   picture without recursion. */
#pragma once
#include <stdint.h>

#define OD_MC_LOG_MVB_MAX 3     /* leaves are 1, 2, 4 or 8 grid steps wide */
#define OD_MC_TOP 2             /* rows / columns of filter support before the sample */
#define OD_MC_APRON 5           /* taps - 1 */
#define OD_MC_BORDER 64         /* luma samples the reference replicates round a coded frame */

/* leaf descriptor: vx | vy << 12 | log size << 24 | outside corner << 26 | split flags << 28 */
#define OD_MC_LEAF(vx, vy, lg, oc, s) \
  ((uint32_t)(vx) | (uint32_t)(vy) << 12 | (uint32_t)(lg) << 24 | (uint32_t)(oc) << 26 | (uint32_t)(s) << 28)
#define OD_MC_LEAF_VX(d) ((int)((d) & 0xfff))
#define OD_MC_LEAF_VY(d) ((int)((d) >> 12 & 0xfff))
#define OD_MC_LEAF_LOG(d) ((int)((d) >> 24 & 3))
#define OD_MC_LEAF_OC(d) ((int)((d) >> 26 & 3))
#define OD_MC_LEAF_S(d) ((int)((d) >> 28 & 3))

/* coded frame sizes the grids serve: whole 64x64 cells, coordinates inside a leaf descriptor's 12 bits */
static inline bool od_mc_size_ok(int coded_w, int coded_h) {
  return coded_w >= 64 && coded_h >= 64 && coded_w%64 == 0 && coded_h%64 == 0 && coded_w <= 32704
   && coded_h <= 32704;
}

/* corner k of a block, clockwise from the upper left, in block units */
__host__ __device__ static inline int od_mc_corner_dx(int k) { return (k == 1) | (k == 2); }
__host__ __device__ static inline int od_mc_corner_dy(int k) { return k >> 1; }

/* The grid point (in leaf-size units from the leaf's upper left) that supplies corner k of a leaf with
   outside corner oc and split flags s.  With both neighbours split (s = 3) these are the block's own
   corners; an unsplit neighbour moves the corner it shares with that neighbour one step further out along
   the shared edge, to the neighbour's own grid point. */
__host__ __device__ static inline void od_mc_vertex(int oc, int s, int k, int *dx, int *dy) {
  int x = od_mc_corner_dx(k);
  int y = od_mc_corner_dy(k);
  /* neighbour (oc + 1) & 3 unsplit (s bit 0 clear) displaces that corner; likewise (oc + 3) & 3 for bit 1 */
  if (!(s & 1) && k == ((oc + 1) & 3)) {
    x += od_mc_corner_dx(k) - od_mc_corner_dx(oc);
    y += od_mc_corner_dy(k) - od_mc_corner_dy(oc);
  }
  if (!(s & 2) && k == ((oc + 3) & 3)) {
    x += od_mc_corner_dx(k) - od_mc_corner_dx(oc);
    y += od_mc_corner_dy(k) - od_mc_corner_dy(oc);
  }
  *dx = x;
  *dy = y;
}

/* Is (vx, vy) the upper-left cell of a leaf?  valid(x, y) reads a grid point's flag. */
template <class V>
__host__ __device__ static inline bool od_mc_leaf_at(V valid, int vx, int vy, uint32_t *desc) {
  int lg = OD_MC_LOG_MVB_MAX;
  for (; lg > 0; lg--) {
    const int m = (1 << lg) - 1;
    const int half = 1 << lg >> 1;
    if (!valid((vx & ~m) + half, (vy & ~m) + half)) break;
  }
  if ((vx | vy) & ((1 << lg) - 1)) return false;
  int oc = 0;
  int s = 3;
  if (lg < OD_MC_LOG_MVB_MAX) {
    const int m = (1 << (lg + 1)) - 1;
    oc = (vx & m) != 0;
    if (vy & m) oc = 3 - oc;
    const int k1 = (oc + 1) & 3;
    const int k3 = (oc + 3) & 3;
    s = (valid(vx + (od_mc_corner_dx(k1) << lg), vy + (od_mc_corner_dy(k1) << lg)) ? 1 : 0)
     | (valid(vx + (od_mc_corner_dx(k3) << lg), vy + (od_mc_corner_dy(k3) << lg)) ? 2 : 0);
  }
  *desc = OD_MC_LEAF(vx, vy, lg, oc, s);
  return true;
}

/* a vector component at a plane's decimation: division by 1 << dec, ties to even */
__host__ __device__ static inline int od_mc_scale_mv(int v, int dec) {
  return (v + (((1 << dec) + (v >> dec & 1) - 1) >> 1)) >> dec;
}

/* One axis of the legal range: does the (blk + 5)-wide filter window of a leaf of 1 << lg grid steps at grid
   position v, moved by the vector component mv (1/8 luma pel), stay inside the border the reference replicates
   round an axis of n grid steps, at a plane's decimation? */
__host__ __device__ static inline bool od_mc_window_ok(int v, int mv, int lg, int dec, int n) {
  const int pad = OD_MC_BORDER >> dec;
  const int blk = 8 << lg >> dec;
  const long x0 = (long)(v << 3 >> dec) + (od_mc_scale_mv(mv, dec) >> 3) - OD_MC_TOP;
  return x0 >= -pad && x0 + blk + OD_MC_APRON <= (n << 3 >> dec) + pad;
}

/* One axis of the motion search's legal range (me_kernels.hip): a component is legal for the point at v of a
   uniform grid of 1 << lg steps when both leaves of that size inside the frame that have the point as a corner
   keep their windows inside the border, in luma and in 4:2:0 chroma.  Monotone in mv, and 0 is always legal. */
__host__ __device__ static inline bool od_me_mv_ok(int v, int mv, int lg, int n) {
  for (int d = 0; d < 2; d++) {
    const int lv = v - (d << lg);
    if (lv < 0 || lv >= n) continue;
    if (!od_mc_window_ok(lv, mv, lg, 0, n) || !od_mc_window_ok(lv, mv, lg, 1, n)) return false;
  }
  return true;
}

/* One axis of the variable-block-size search's legal range (odhip_me_search_vbs): a component is legal for the
   point at v, of whatever size, when a leaf of 1 << lg_top steps at the origin of every cell of that size inside the
   frame whose closed extent holds v keeps its window inside the border, in luma and in 4:2:0 chroma.  Every leaf of a
   grid of leaves up to that size that reads the point lies inside such a cell and its window inside the cell's.  At
   a multiple of the size this is od_me_mv_ok at that size.  Monotone in mv, and 0 is always legal. */
__host__ __device__ static inline bool od_me_mv_ok_cells(int v, int mv, int lg_top, int n) {
  const int m = (1 << lg_top) - 1;
  for (int d = 0; d < 2; d++) {
    if (d && (v & m)) break;                 /* inside a cell: that cell alone */
    const int c = (v & ~m) - (d << lg_top);
    if (c < 0 || c >= n) continue;
    if (!od_mc_window_ok(c, mv, lg_top, 0, n) || !od_mc_window_ok(c, mv, lg_top, 1, n)) return false;
  }
  return true;
}
