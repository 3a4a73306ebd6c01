/* mc_filter.cuh - one vector's prediction of a block: the reference's separable 6-tap interpolation at 1/8 pel
   (od_mc_predict1fmv8_c / od_mc_predict1fmv16_c, src/mc.c:94-340), shared by the motion compensation
   (mc_kernels.hip) and the motion search (me_kernels.hip).  Integer only; every intermediate has the
   reference's width: the 8-bit variant keeps its first pass in int16, the full-precision one in int32. */
#pragma once
#include <stdint.h>
#include "mc_walk.cuh"

namespace {

constexpr int kTaps = 6;
constexpr int kTop = OD_MC_TOP;
constexpr int kApron = OD_MC_APRON;
constexpr int kScale = 7;        /* the filters sum to 1 << kScale */
constexpr int kFprShift = 4;     /* full-precision planes: 8 + 4 bits */

/* windowed-sinc interpolation filters by eighth-pel phase, taps for samples -2 .. +3 */
__constant__ int16_t c_subpel[8][kTaps] = {
  {0, 0, 128, 0, 0, 0}, {1, -9, 122, 18, -5, 1}, {3, -15, 112, 37, -11, 2}, {3, -18, 97, 58, -15, 3},
  {4, -20, 80, 80, -20, 4}, {3, -15, 58, 97, -18, 3}, {2, -11, 37, 112, -15, 3}, {1, -5, 18, 122, -9, 1}};

template <class T> struct McTraits;
template <> struct McTraits<uint8_t> {
  typedef int16_t mid_t;
  static __device__ inline int hfilt(int sum) { return sum - (128 << kScale); }
  static __device__ inline int hcopy(int v) { return (v << kScale) - (128 << kScale); }
  static __device__ inline uint8_t vfilt(int sum) {
    return clamp((sum + (1 << (2*kScale - 1)) + (128 << 2*kScale)) >> 2*kScale);
  }
  static __device__ inline uint8_t vcopy(int v) {
    return clamp((v + (1 << (kScale - 1)) + (128 << kScale)) >> kScale);
  }
  static __device__ inline uint8_t clamp(int x) { return (uint8_t)(x < 0 ? 0 : x > 255 ? 255 : x); }
};
template <> struct McTraits<int16_t> {
  typedef int32_t mid_t;
  static constexpr int kMid = 128 << kFprShift;
  static constexpr int kMax = (1 << (8 + kFprShift)) - 1;
  static __device__ inline int hfilt(int sum) { return sum - (128 << (kFprShift + kScale)); }
  static __device__ inline int hcopy(int v) { return (v - kMid)*(1 << kScale); }
  static __device__ inline int16_t vfilt(int sum) {
    return clamp(((sum + (1 << 2*kScale >> 1)) >> 2*kScale) + kMid);
  }
  static __device__ inline int16_t vcopy(int v) { return clamp(((v + (1 << kScale >> 1)) >> kScale) + kMid); }
  static __device__ inline int16_t clamp(int x) { return (int16_t)(x < 0 ? 0 : x > kMax ? kMax : x); }
};

/* First pass at phase fx: row points at the sample kTop to the left of the one interpolated.  The caller
   stores the result as mid_t. */
template <class T>
__device__ inline int mc_hpass(const T *row, int fx) {
  if (!fx) return McTraits<T>::hcopy(row[kTop]);
  int sum = 0;
#pragma unroll
  for (int t = 0; t < kTaps; t++) sum += row[t]*c_subpel[fx][t];
  return McTraits<T>::hfilt(sum);
}

/* Second pass at phase fy over first-pass values `stride` apart: col points at the row kTop above. */
template <class T>
__device__ inline T mc_vpass(const typename McTraits<T>::mid_t *col, int stride, int fy) {
  if (!fy) return McTraits<T>::vcopy(col[kTop*stride]);
  int sum = 0;
#pragma unroll
  for (int t = 0; t < kTaps; t++) sum += col[t*stride]*c_subpel[fy][t];
  return McTraits<T>::vfilt(sum);
}

}  // namespace
