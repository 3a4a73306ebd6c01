/* od_cfl.cuh - the 4x4 luma case of od_resample_luma_coeffs (src/intra.c:77-93), shared by the kernels that
   build chroma-from-luma reference planes from pulses (k_cfl_ref_tf, pvq_bands.hip) and from dequantised
   planes at a block-size map (k_cfl_part, partition_kernels.hip, and its host entry point). */
#pragma once
#include <hip/hip_runtime.h>

/* Coefficient (i, j), i, j < 4, of the 4x4 chroma block over an 8x8 luma area of four 4x4 blocks:
   od_tf_up_hv_lp (src/tf.c:82-108) merges coefficient (i >> 1, j >> 1) of the upper-left (ll), upper-right
   (lh), lower-left (hl) and lower-right (hh) block with OD_HAAR_KERNEL(ll, hl, lh, hh) (src/tf.h:34-45; lh and
   hl swapped, src/tf.c:99-100) and places the four outputs in the 2x2 group at (2*(i >> 1), 2*(j >> 1)),
   swapped by the group's parity; OD_CFL_SCALING4 (src/intra.c:65-70), indexed [column][row] (:92), scales it.
   Both shifts are arithmetic. */
__host__ __device__ inline int od_cfl_tf4(int ll, int lh, int hl, int hh, int i, int j) {
  constexpr short scaling4[4][4] = {{128, 128, 100, 36}, {128, 80, 71, 35}, {100, 71, 35, 31}, {36, 35, 31, 18}};
  ll += lh;
  hh -= hl;
  const int t = (ll - hh) >> 1;
  hl = t - hl;
  lh = t - lh;
  ll -= hl;
  hh += lh;
  const bool row_first = (i & 1) == ((i >> 1) & 1);     /* rows 2y + vswap hold ll / lh */
  const bool col_first = (j & 1) == ((j >> 1) & 1);     /* columns 2x + hswap hold ll / hl */
  const int v = row_first ? (col_first ? ll : lh) : (col_first ? hl : hh);
  return (scaling4[j][i]*v + 64) >> 7;
}
