/* od_sample.cuh - the samples of an odhip_metrics_pair, shared by the metric kernels (metrics_kernels.hip,
   msssim_kernels.hip, fastssim_kernels.hip): one sample of a plane in any ODHIP_SAMPLE_* format, and the checks of a pair. */
#pragma once
#include "../../include/daala_hip.h"
#include "od_common.cuh"

namespace {

/* ODHIP_SAMPLE_I16_12 goes through the reference's output conversion: rounded to the depth and clamped */
__device__ __forceinline__ int load_sample(const void *base, int fmt, int stride, int x, int y, int depth) {
  const long at = (long)y*stride + x;
  if (fmt == ODHIP_SAMPLE_U8) return static_cast<const uint8_t *>(base)[at];
  if (fmt == ODHIP_SAMPLE_U16) return static_cast<const uint16_t *>(base)[at];
  const int sh = 12 - depth;
  const int v = (static_cast<const int16_t *>(base)[at] + (1 << sh >> 1)) >> sh;
  return min(max(v, 0), (1 << depth) - 1);
}

inline bool fmt_ok(int fmt, int depth) {
  return (fmt == ODHIP_SAMPLE_U8 && depth == 8) || fmt == ODHIP_SAMPLE_U16 || fmt == ODHIP_SAMPLE_I16_12;
}

inline bool pair_ok(const odhip_metrics_pair &q) {
  return q.src && q.rec && q.w > 0 && q.h > 0 && q.w <= 65535 && q.h <= 65535 && q.src_stride >= q.w
   && q.rec_stride >= q.w && (q.depth == 8 || q.depth == 10 || q.depth == 12) && fmt_ok(q.src_fmt, q.depth)
   && fmt_ok(q.rec_fmt, q.depth) && q.csf >= ODHIP_CSF_Y && q.csf <= ODHIP_CSF_CR;
}

}  // namespace
