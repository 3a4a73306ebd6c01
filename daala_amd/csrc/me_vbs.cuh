/* me_vbs.cuh - the decision and the point rule of the variable-block-size motion search (odhip_me_search_vbs,
   me_kernels.hip; include/daala_hip.h has the definition), shared by its kernels and any host-side restatement.

   A 64x64 cell's decisions are 21 bits: does the cell split, do its four 32x32 quadrants, do its sixteen 16x16 cells.
   A bit is the bare comparison of two distortions (od_vbs_split) and reads no neighbour.  The `valid` pattern that
   follows from the bits is the one the grid's rule allows (mc_walk.cuh; A: points at multiples of 8 steps are valid,
   B: a centre only between four valid corners, C: an edge midpoint only between valid ends and split cells), with
   every point the rule allows and the bits ask for.  It has a closed form with no state and no order:
     S_3(c) = bit(c)
     S_lg(c) = bit(c) and S_lg+1(parent of c) and S_lg+1 of the two cells of the parent's size across c's two outer
               edges of the parent                         (c's corners are the parent's corner, centre and two edge
                                                            midpoints; a cell outside the frame counts as split)
     an edge midpoint of size lg is valid iff S_lg of both cells that share the edge (its ends are their corners)
   so a point's flag costs at most 26 bit reads and a launch needs no pass per size. */
#pragma once
#include "mc_walk.cuh"

/* the bit of the cell of 1 << lg steps (lg 1 .. 3) that holds the 8x8 cell (x, y) of a 64x64 cell, x, y in 0 .. 7 */
__host__ __device__ static inline int od_vbs_bit(int lg, int x, int y) {
  return lg == 3 ? 0 : lg == 2 ? 1 + 2*(y >> 2) + (x >> 2) : 5 + 4*(y >> 1) + (x >> 1);
}

/* The decision: a cell splits iff its quadrants' summed distortion, plus the penalty, is strictly below its own.
   D <= 64*64*255 and the penalty <= 2^24: 64 bits hold it with room. */
__host__ __device__ static inline bool od_vbs_split(uint32_t d_small, uint32_t d_big, int penalty) {
  return 8ll*d_small + penalty < 8ll*d_big;
}

/* S_LG of the cell of 1 << LG steps that holds the 8x8 cell (x, y): is its centre valid?  bits(cx, cy) gives the
   decisions of the 64x64 cell (cx, cy) inside the frame; a cell outside the frame counts as split. */
template <int LG, class B>
__host__ __device__ static inline bool od_vbs_centre(B bits, int x, int y, int nh, int nv) {
  if (x < 0 || x >= nh || y < 0 || y >= nv) return true;
  if (!(bits(x >> 3, y >> 3) >> od_vbs_bit(LG, x & 7, y & 7) & 1)) return false;
  if constexpr (LG < 3) {
    const int size = 2 << LG;                /* the parent's */
    const int px = x & ~(size - 1);
    const int py = y & ~(size - 1);
    const int nx = x & (1 << LG) ? px + size : px - 1;
    const int ny = y & (1 << LG) ? py + size : py - 1;
    return od_vbs_centre<LG + 1>(bits, x, y, nh, nv) && od_vbs_centre<LG + 1>(bits, nx, y, nh, nv)
     && od_vbs_centre<LG + 1>(bits, x, ny, nh, nv);
  }
  else return true;
}

template <class B>
__host__ __device__ static inline bool od_vbs_centre_at(B bits, int lg, int x, int y, int nh, int nv) {
  return lg == 3 ? od_vbs_centre<3>(bits, x, y, nh, nv) : lg == 2 ? od_vbs_centre<2>(bits, x, y, nh, nv)
   : od_vbs_centre<1>(bits, x, y, nh, nv);
}

/* the `valid` flag of grid point (x, y), 0 <= x <= nh, 0 <= y <= nv */
template <class B>
__host__ __device__ static inline bool od_vbs_point_valid(B bits, int x, int y, int nh, int nv) {
  int tz = 0;
  while (tz < 3 && !((x | y) >> tz & 1)) tz++;
  if (tz == 3) return true;
  const int lg = tz + 1;                     /* the point is a centre or an edge midpoint of cells of this size */
  const bool ox = (x >> tz & 1) != 0;
  const bool oy = (y >> tz & 1) != 0;
  if (ox && oy) return od_vbs_centre_at(bits, lg, x, y, nh, nv);
  if (ox) return od_vbs_centre_at(bits, lg, x, y - 1, nh, nv) && od_vbs_centre_at(bits, lg, x, y, nh, nv);
  return od_vbs_centre_at(bits, lg, x - 1, y, nh, nv) && od_vbs_centre_at(bits, lg, x, y, nh, nv);
}

/* log size of the leaf that covers the 8x8 cell (x, y) inside the frame: the walk of od_mc_leaf_at */
template <class B>
__host__ __device__ static inline int od_vbs_leaf_log(B bits, int x, int y, int nh, int nv) {
  if (!od_vbs_centre<3>(bits, x, y, nh, nv)) return 3;
  if (!od_vbs_centre<2>(bits, x, y, nh, nv)) return 2;
  return od_vbs_centre<1>(bits, x, y, nh, nv) ? 0 : 1;
}

/* The size a valid point takes its record from: the log size of the smallest leaf that has the point among its own
   four corners - a leaf that has the point as a corner holds one of the four 8x8 cells round it, and is aligned to
   its size.  4 when there is none. */
template <class B>
__host__ __device__ static inline int od_vbs_point_size(B bits, int x, int y, int nh, int nv) {
  int s = 4;
  for (int k = 0; k < 4; k++) {
    const int cx = x - (k & 1);
    const int cy = y - (k >> 1);
    if (cx < 0 || cx >= nh || cy < 0 || cy >= nv) continue;
    const int lg = od_vbs_leaf_log(bits, cx, cy, nh, nv);
    if (!((x | y) & ((1 << lg) - 1)) && lg < s) s = lg;
  }
  return s;
}
