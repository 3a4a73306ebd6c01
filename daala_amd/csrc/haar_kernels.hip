/* haar_kernels.hip - the encoder's second coefficient path: lossless and Haar-wavelet frames.

   With use_haar_wavelet set (always when lossless, src/encode.c:3027) a frame skips the lapped filters, the DCTs
   and PVQ: every superblock is one block (:3087-3088), transformed with the reversible integer Haar wavelet
   (od_haar / od_haar_inv, src/dct.c:4822-4888), quantised per sub-band (od_wavelet_quantize, src/encode.c:1003-1080,
   OD_HAAR_QM src/state.c:55-60) and coded as three trees of magnitude sums (od_compute_max_tree :899-919).  Integers
   only: no margin, no replay.

   k_haar_forward   one workgroup per block: samples converted on load into an LDS tile (a second one for the
                    prediction when inter), od_haar fine to coarse IN PLACE - a level's quads are read into
                    registers, a barrier, then its LL and its three sub-bands are written where od_haar puts
                    them, the sub-bands already quantised, their tree sums (own magnitude + the four children of
                    the level before) into a second tile; whole 16-byte row segments out.
   k_haar_dc        keyframes: the superblock-DC predictor (od_quantize_haar_dc_sb, src/encode.c:1537-1590), one
                    workgroup per plane, one lane walking the plane's DCs in raster order; encoder and decoder.
   k_haar_inverse   dequantiser (:1065-1078), od_haar_inv coarse to fine in LDS, od_coeff_to_ref_buf.
   k_haar_planes    the bare transforms of coefficient planes (test surface).  */
#include <stdint.h>
#include <string.h>
#include "od_buf.cuh"
#include "od_ctx.cuh"

namespace {

constexpr int kNT = 256;
/* superblock DCs of a plane that k_haar_dc stages in LDS (twice: symbols and reconstructions); a plane with more
   walks in global memory */
constexpr int kDcLds = 2048;
constexpr int kMaxQuant = 1 << 20;
constexpr int kMaxDcQuant = 1 << 24;

/* OD_HAAR_QM, src/state.c:55-60: [dir == 2][level from LF] */
const int kHaarQm[2][6] = {{16, 16, 16, 16, 24, 32}, {16, 16, 16, 24, 32, 48}};

/* A divisor and floor(2^32 / q) (2^32 - 1 for q == 1), prepared by the host. */
struct HaarDiv {
  uint32_t q;
  uint32_t m;
};

struct HaarArgs {
  const void *px;
  const void *pred;
  void *rec;
  int *q;
  int *tree;
  int *dc_rec;            /* [nplanes][nvsb*nhsb]; never null inside a launch that uses it */
  int *dc_sym;            /* k_haar_dc beyond its LDS budget: [nplanes][nvsb*nhsb] */
  long px_plane_stride;
  int px_stride;
  int w, h;
  int pic_w, pic_h;
  int shift;              /* 8-bit samples: coefficient = (s - 128) << shift; int16: (s - 2048 + round) >> shift */
  int plane_split;
  int encode;             /* k_haar_dc: DCs to symbols, else symbols to DCs */
  HaarDiv ac[2][6];       /* [dir == 2][level from LF] */
  HaarDiv dc[2];
};

inline HaarDiv make_div(int q) {
  HaarDiv d;
  d.q = (uint32_t)q;
  d.m = q == 1 ? 0xffffffffu : (uint32_t)((1ull << 32)/(uint32_t)q);
  return d;
}

/* OD_DIV_R0 (src/odintrin.h:123), exact for every int32 x and 1 <= q < 2^31: n = |x| + ((q + 1 >> 1) - 1) < 2^32,
   the estimate umulhi(n, m) is floor(n/q) or one below it (n*(2^32/q - m) < 2^32), one correction settles it. */
__device__ __forceinline__ int div_r0(int x, HaarDiv d) {
  const uint32_t n = (uint32_t)abs(x) + ((d.q - 1) >> 1);
  uint32_t e = __umulhi(n, d.m);
  e += (n - e*d.q >= d.q) ? 1u : 0u;
  return x < 0 ? -(int)e : (int)e;
}

/* OD_HAAR_KERNEL, src/tf.h:34-45 */
__device__ __forceinline__ void haar_kernel(int &ll, int &lh, int &hl, int &hh) {
  ll += hl;
  hh -= lh;
  const int t = (ll - hh) >> 1;
  lh = t - lh;
  hl = t - hl;
  ll -= lh;
  hh += hl;
}

template <class T>
struct Vec4 {
  typedef T type __attribute__((ext_vector_type(4)));
};

/* od_ref_buf_to_coeff, src/state.c:1216-1255: the 8-bit branch (shift = depth - 8 lossless, OD_COEFF_SHIFT lossy)
   and the full-precision branch (shift = OD_COEFF_SHIFT - (depth - 8) lossless, 0 lossy) */
__device__ __forceinline__ int to_coeff(uint8_t s, int shift) {
  return ((int)s - 128)*(1 << shift);
}
__device__ __forceinline__ int to_coeff(int16_t s, int shift) {
  return ((int)s - 2048 + (1 << shift >> 1)) >> shift;
}
/* od_coeff_to_ref_buf, src/state.c:1281-1323, with OD_CLAMP255 / OD_CLAMPFPR */
__device__ __forceinline__ void to_sample(uint8_t &out, int c, int shift) {
  out = (uint8_t)min(max(((c + (1 << shift >> 1)) >> shift) + 128, 0), 255);
}
__device__ __forceinline__ void to_sample(int16_t &out, int c, int shift) {
  out = (int16_t)min(max(c*(1 << shift) + 2048, 0), 4095);
}

__device__ __forceinline__ int sum4(const int *s, int n, int y, int x) {
  const int2 a = *reinterpret_cast<const int2 *>(s + y*n + x);
  const int2 b = *reinterpret_cast<const int2 *>(s + (y + 1)*n + x);
  return a.x + a.y + b.x + b.y;
}

/* What the last level leaves in thread 0: the block's DC, its prediction's, the three tree roots. */
struct HaarTop {
  int dc, pdc, t0, t1, t2;
};

/* Level L (0 = finest) of od_haar on the N x N tile s_c, in place; with INTER the same on s_p.  QUANT: the three
   sub-bands are stored quantised (OD_DIV_R0 of coefficient - prediction, src/encode.c:1012-1027), their tree sums
   (od_compute_max_tree, :899-919) into s_t.  Then the levels above. */
template <int LN, int L, int NT, bool QUANT, bool INTER>
__device__ __forceinline__ void fwd_levels(int *s_c, int *s_p, int *s_t, const HaarArgs &a, int tid, HaarTop &top) {
  constexpr int N = 1 << LN;
  constexpr int NP = N >> (L + 1);
  constexpr int CNT = NP*NP;
  constexpr int K = (CNT + NT - 1)/NT;
  constexpr int LVL = LN - 1 - L;          /* the reference counts levels from LF */
  int ca[K], cb[K], cc[K], cd[K];
  int pa[K], pb[K], pc[K], pd[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int idx = tid + k*NT;
    if (idx < CNT) {
      const int i = idx/NP;
      const int j = idx%NP;
      const int2 t = *reinterpret_cast<const int2 *>(s_c + 2*i*N + 2*j);
      const int2 u = *reinterpret_cast<const int2 *>(s_c + (2*i + 1)*N + 2*j);
      ca[k] = t.x;
      cb[k] = u.x;          /* b is the sample BELOW a */
      cc[k] = t.y;
      cd[k] = u.y;
      haar_kernel(ca[k], cb[k], cc[k], cd[k]);
      if (INTER) {
        const int2 v = *reinterpret_cast<const int2 *>(s_p + 2*i*N + 2*j);
        const int2 w = *reinterpret_cast<const int2 *>(s_p + (2*i + 1)*N + 2*j);
        pa[k] = v.x;
        pb[k] = w.x;
        pc[k] = v.y;
        pd[k] = w.y;
        haar_kernel(pa[k], pb[k], pc[k], pd[k]);
      } else {
        pa[k] = pb[k] = pc[k] = pd[k] = 0;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int idx = tid + k*NT;
    if (idx < CNT) {
      const int i = idx/NP;
      const int j = idx%NP;
      s_c[i*N + j] = ca[k];
      if (INTER) s_p[i*N + j] = pa[k];
      int b = cb[k], c = cc[k], d = cd[k];
      if (QUANT) {
        b = div_r0(b - pb[k], a.ac[0][LVL]);
        c = div_r0(c - pc[k], a.ac[0][LVL]);
        d = div_r0(d - pd[k], a.ac[1][LVL]);
        int tb = abs(b), tc = abs(c), td = abs(d);
        if (L > 0) {
          tb += sum4(s_t, N, 2*i, 2*(j + NP));
          tc += sum4(s_t, N, 2*(i + NP), 2*j);
          td += sum4(s_t, N, 2*(i + NP), 2*(j + NP));
        }
        s_t[i*N + j + NP] = tb;
        s_t[(i + NP)*N + j] = tc;
        s_t[(i + NP)*N + j + NP] = td;
        if (L == LN - 1) {
          top.t0 = tb;
          top.t1 = tc;
          top.t2 = td;
        }
      }
      s_c[i*N + j + NP] = b;
      s_c[(i + NP)*N + j] = c;
      s_c[(i + NP)*N + j + NP] = d;
      if (L == LN - 1) {
        top.dc = ca[k];
        top.pdc = pa[k];
      }
    }
  }
  __syncthreads();
  if constexpr (L + 1 < LN) fwd_levels<LN, L + 1, NT, QUANT, INTER>(s_c, s_p, s_t, a, tid, top);
}

/* Level L of od_haar_inv on the tile s_c, in place, then the levels below it (coarse to fine).  DEQ: the sub-bands
   hold quantised values, dequantised as they are read (q*x + prediction, src/encode.c:1065-1078). */
template <int LN, int L, int NT, bool DEQ, bool INTER>
__device__ __forceinline__ void inv_levels(int *s_c, const int *s_p, const HaarArgs &a, int tid) {
  constexpr int N = 1 << LN;
  constexpr int NP = N >> (L + 1);
  constexpr int CNT = NP*NP;
  constexpr int K = (CNT + NT - 1)/NT;
  constexpr int LVL = LN - 1 - L;
  int ca[K], cb[K], cc[K], cd[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int idx = tid + k*NT;
    if (idx < CNT) {
      const int i = idx/NP;
      const int j = idx%NP;
      ca[k] = s_c[i*N + j];
      cb[k] = s_c[i*N + j + NP];
      cc[k] = s_c[(i + NP)*N + j];
      cd[k] = s_c[(i + NP)*N + j + NP];
      if (DEQ) {
        cb[k] *= (int)a.ac[0][LVL].q;
        cc[k] *= (int)a.ac[0][LVL].q;
        cd[k] *= (int)a.ac[1][LVL].q;
        if (INTER) {
          cb[k] += s_p[i*N + j + NP];
          cc[k] += s_p[(i + NP)*N + j];
          cd[k] += s_p[(i + NP)*N + j + NP];
        }
      }
      haar_kernel(ca[k], cb[k], cc[k], cd[k]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int idx = tid + k*NT;
    if (idx < CNT) {
      const int i = idx/NP;
      const int j = idx%NP;
      *reinterpret_cast<int2 *>(s_c + 2*i*N + 2*j) = make_int2(ca[k], cc[k]);
      *reinterpret_cast<int2 *>(s_c + (2*i + 1)*N + 2*j) = make_int2(cb[k], cd[k]);
    }
  }
  __syncthreads();
  if constexpr (L > 0) inv_levels<LN, L - 1, NT, DEQ, INTER>(s_c, s_p, a, tid);
}

/* Rows of four samples of the block at (bx, by) of plane p into the tile, converted; INTER: the prediction's too, and
   source samples outside the picture replaced by the prediction's (src/encode.c:2589-2602). */
template <int LN, class T, bool INTER>
__device__ __forceinline__ void load_samples(int *s_c, int *s_p, const HaarArgs &a, bool want_src, int tid) {
  constexpr int N = 1 << LN;
  typedef typename Vec4<T>::type V;
  const long at = (long)blockIdx.z*a.px_plane_stride + (long)blockIdx.y*N*a.px_stride + blockIdx.x*N;
  for (int g = tid; g < N*N/4; g += kNT) {
    const int y = g/(N/4);
    const int x = g%(N/4)*4;
    const long off = at + (long)y*a.px_stride + x;
    V pv = {};
    if (INTER) {
      pv = *reinterpret_cast<const V *>(static_cast<const T *>(a.pred) + off);
      int4 c;
      c.x = to_coeff(pv.x, a.shift);
      c.y = to_coeff(pv.y, a.shift);
      c.z = to_coeff(pv.z, a.shift);
      c.w = to_coeff(pv.w, a.shift);
      *reinterpret_cast<int4 *>(s_p + y*N + x) = c;
    }
    if (want_src) {
      V v = *reinterpret_cast<const V *>(static_cast<const T *>(a.px) + off);
      if (INTER) {
        const int gx = blockIdx.x*N + x;
        const bool below = blockIdx.y*N + y >= a.pic_h;
        if (below || gx + 0 >= a.pic_w) v.x = pv.x;
        if (below || gx + 1 >= a.pic_w) v.y = pv.y;
        if (below || gx + 2 >= a.pic_w) v.z = pv.z;
        if (below || gx + 3 >= a.pic_w) v.w = pv.w;
      }
      int4 c;
      c.x = to_coeff(v.x, a.shift);
      c.y = to_coeff(v.y, a.shift);
      c.z = to_coeff(v.z, a.shift);
      c.w = to_coeff(v.w, a.shift);
      *reinterpret_cast<int4 *>(s_c + y*N + x) = c;
    }
  }
}

template <int LN, class T, bool INTER>
__global__ __launch_bounds__(kNT) void k_haar_forward(const HaarArgs a) {
  constexpr int N = 1 << LN;
  __shared__ __attribute__((aligned(16))) int s_c[N*N];
  __shared__ __attribute__((aligned(16))) int s_t[N*N];
  __shared__ __attribute__((aligned(16))) int s_p[INTER ? N*N : 4];
  const int tid = threadIdx.x;
  load_samples<LN, T, INTER>(s_c, s_p, a, true, tid);
  __syncthreads();
  HaarTop top = {};
  fwd_levels<LN, 0, kNT, true, INTER>(s_c, s_p, s_t, a, tid, top);
  if (tid == 0) {
    /* tree_sum[0][0], src/encode.c:1033 */
    s_t[0] = top.t0 + top.t1 + top.t2;
    if (INTER) {
      /* src/encode.c:1337-1343, :1373-1374 */
      const HaarDiv dq = a.dc[(int)blockIdx.z >= a.plane_split ? 1 : 0];
      const int diff = top.dc - top.pdc;
      const int sym = abs(diff) < (int)((long long)dq.q*141/256) ? 0 : div_r0(diff, dq);
      s_c[0] = sym;
      if (a.dc_rec) {
        a.dc_rec[((long)blockIdx.z*gridDim.y + blockIdx.y)*gridDim.x + blockIdx.x] = sym*(int)dq.q + top.pdc;
      }
    }
    /* a keyframe's DC goes out as it is: k_haar_dc turns it into its symbol */
  }
  __syncthreads();
  const long at = ((long)blockIdx.z*a.h + (long)blockIdx.y*N)*a.w + blockIdx.x*N;
  for (int g = tid; g < N*N/4; g += kNT) {
    const int y = g/(N/4);
    const int x = g%(N/4)*4;
    const long off = at + (long)y*a.w + x;
    *reinterpret_cast<int4 *>(a.q + off) = *reinterpret_cast<const int4 *>(s_c + y*N + x);
    *reinterpret_cast<int4 *>(a.tree + off) = *reinterpret_cast<const int4 *>(s_t + y*N + x);
  }
}

template <int LN, class T, bool INTER>
__global__ __launch_bounds__(kNT) void k_haar_inverse(const HaarArgs a) {
  constexpr int N = 1 << LN;
  typedef typename Vec4<T>::type V;
  __shared__ __attribute__((aligned(16))) int s_c[N*N];
  __shared__ __attribute__((aligned(16))) int s_p[INTER ? N*N : 4];
  const int tid = threadIdx.x;
  const long at = ((long)blockIdx.z*a.h + (long)blockIdx.y*N)*a.w + blockIdx.x*N;
  for (int g = tid; g < N*N/4; g += kNT) {
    const int y = g/(N/4);
    const int x = g%(N/4)*4;
    *reinterpret_cast<int4 *>(s_c + y*N + x) = *reinterpret_cast<const int4 *>(a.q + at + (long)y*a.w + x);
  }
  if (INTER) {
    /* predt again from the prediction's samples, not from a stored plane */
    load_samples<LN, T, INTER>(s_c, s_p, a, false, tid);
    __syncthreads();
    HaarTop top = {};
    fwd_levels<LN, 0, kNT, false, false>(s_p, nullptr, nullptr, a, tid, top);
  } else {
    __syncthreads();
  }
  if (tid == 0) {
    const long sb = ((long)blockIdx.z*gridDim.y + blockIdx.y)*gridDim.x + blockIdx.x;
    if (INTER) {
      /* src/decode.c:574; the decoder has no forward kernel to leave the reconstructed DC behind */
      s_c[0] = s_c[0]*(int)a.dc[(int)blockIdx.z >= a.plane_split ? 1 : 0].q + s_p[0];
      if (a.dc_rec) a.dc_rec[sb] = s_c[0];
    } else {
      s_c[0] = a.dc_rec[sb];
    }
  }
  __syncthreads();
  inv_levels<LN, LN - 1, kNT, true, INTER>(s_c, s_p, a, tid);
  const long pat = (long)blockIdx.z*a.px_plane_stride + (long)blockIdx.y*N*a.px_stride + blockIdx.x*N;
  for (int g = tid; g < N*N/4; g += kNT) {
    const int y = g/(N/4);
    const int x = g%(N/4)*4;
    const int4 c = *reinterpret_cast<const int4 *>(s_c + y*N + x);
    T s0, s1, s2, s3;
    to_sample(s0, c.x, a.shift);
    to_sample(s1, c.y, a.shift);
    to_sample(s2, c.z, a.shift);
    to_sample(s3, c.w, a.shift);
    V v;
    v.x = s0;
    v.y = s1;
    v.z = s2;
    v.w = s3;
    *reinterpret_cast<V *>(static_cast<T *>(a.rec) + pat + (long)y*a.px_stride + x) = v;
  }
}

/* od_quantize_haar_dc_sb (src/encode.c:1537-1590) over a plane's superblocks in raster order, the decoder's
   od_decode_haar_dc_sb the same with the symbol given: the one walk, by one lane.  sym holds the DCs (encode) or their
   symbols, rec receives the reconstructions; both LDS or both global memory - inlined at either, so that the
   compiler knows which. */
__device__ __forceinline__ void dc_walk(int *rec, int *sym, int nhsb, int nvsb, HaarDiv dq, bool encode) {
  const int dc_quant = (int)dq.q;
  for (int by = 0; by < nvsb; by++) {
    int left = 0, upleft = 0, up = 0;
    if (by > 0) up = rec[(by - 1)*nhsb];
    for (int bx = 0; bx < nhsb; bx++) {
      const int idx = by*nhsb + bx;
      const bool has_ur = by > 0 && bx < nhsb - 1;           /* src/encode.c:2640 */
      const int upright = has_ur ? rec[idx - nhsb + 1] : 0;
      int pred;
      if (by > 0 && bx > 0) {
        if (has_ur) pred = (22*left - 9*upleft + 15*up + 4*upright + 16) >> 5;
        else pred = (23*left - 10*upleft + 19*up + 16) >> 5;
      }
      else if (by > 0) pred = up;
      else if (bx > 0) pred = left;
      else pred = 0;
      int v = sym[idx];
      if (encode) {
        v = div_r0(v - pred, dq);
        sym[idx] = v;
      }
      left = v*dc_quant + pred;
      rec[idx] = left;
      upleft = up;
      up = upright;
    }
  }
}

/* One workgroup per plane.  The DC slots of a.q hold the DCs (encode) or their symbols; they are staged in LDS, or
   in global memory beyond kDcLds superblocks, walked, and the symbols (encode) and reconstructions put back. */
__global__ __launch_bounds__(kNT) void k_haar_dc(const HaarArgs a, int tile) {
  __shared__ int s_rec[kDcLds];
  __shared__ int s_sym[kDcLds];
  const int tid = threadIdx.x;
  const int p = blockIdx.x;
  const int nhsb = a.w/tile;
  const int nvsb = a.h/tile;
  const int nsb = nhsb*nvsb;
  int *q = a.q + (long)p*a.w*a.h;
  int *g_rec = a.dc_rec + (long)p*nsb;
  int *g_sym = a.dc_sym + (long)p*nsb;
  const HaarDiv dq = a.dc[p >= a.plane_split ? 1 : 0];
  const bool in_lds = nsb <= kDcLds;
  for (int i = tid; i < nsb; i += kNT) {
    const int v = q[(long)(i/nhsb)*tile*a.w + (i%nhsb)*tile];
    if (in_lds) s_sym[i] = v;
    else g_sym[i] = v;
  }
  __syncthreads();
  if (tid == 0) {
    if (in_lds) dc_walk(s_rec, s_sym, nhsb, nvsb, dq, a.encode != 0);
    else dc_walk(g_rec, g_sym, nhsb, nvsb, dq, a.encode != 0);
  }
  __syncthreads();
  for (int i = tid; i < nsb; i += kNT) {
    if (a.encode) q[(long)(i/nhsb)*tile*a.w + (i%nhsb)*tile] = in_lds ? s_sym[i] : g_sym[i];
    if (in_lds) g_rec[i] = s_rec[i];
  }
}

/* od_haar / od_haar_inv of every N x N block of coefficient planes, one workgroup per block. */
template <int LN, int NT>
__global__ __launch_bounds__(NT) void k_haar_planes(int *out, const int *in, int w, int h, int inverse) {
  constexpr int N = 1 << LN;
  __shared__ __attribute__((aligned(16))) int s_c[N*N];
  const int tid = threadIdx.x;
  const long at = ((long)blockIdx.z*h + (long)blockIdx.y*N)*w + blockIdx.x*N;
  for (int g = tid; g < N*N/4; g += NT) {
    const int y = g/(N/4);
    const int x = g%(N/4)*4;
    *reinterpret_cast<int4 *>(s_c + y*N + x) = *reinterpret_cast<const int4 *>(in + at + (long)y*w + x);
  }
  __syncthreads();
  HaarArgs none = {};
  if (inverse) {
    inv_levels<LN, LN - 1, NT, false, false>(s_c, nullptr, none, tid);
  } else {
    HaarTop top = {};
    fwd_levels<LN, 0, NT, false, false>(s_c, nullptr, nullptr, none, tid, top);
  }
  for (int g = tid; g < N*N/4; g += NT) {
    const int y = g/(N/4);
    const int x = g%(N/4)*4;
    *reinterpret_cast<int4 *>(out + at + (long)y*w + x) = *reinterpret_cast<const int4 *>(s_c + y*N + x);
  }
}

struct HaarState {
  DeviceBuf<int> dc;      /* [2][nplanes][nvsb*nhsb]: reconstructed DCs when the job has no d_dc_rec, k_haar_dc's symbols */
};

bool planes_ok(const void *p, int align) {
  return !((uintptr_t)p & (uintptr_t)(align - 1));
}

/* Everything that does not depend on the context. */
int haar_check(const odhip_haar_job *j, bool encode) {
  if (!j || !j->d_q) return ODHIP_EINVAL;
  if (encode ? !j->d_px || !j->d_tree : !j->d_rec) return ODHIP_EINVAL;
  if (j->nplanes <= 0 || (j->dec != 0 && j->dec != 1)) return ODHIP_EINVAL;
  const int tile = 64 >> j->dec;
  /* the launch grid is (w/tile, h/tile, nplanes) */
  if (j->nplanes > 65535 || j->h/tile > 65535) return ODHIP_EINVAL;
  if (j->w <= 0 || j->h <= 0 || j->w%tile || j->h%tile) return ODHIP_EINVAL;
  if (j->depth != 8 && j->depth != 10 && j->depth != 12) return ODHIP_EINVAL;
  if (j->quant < 0 || j->quant > kMaxQuant || (j->lossless ? j->quant != 0 : j->quant == 0)) return ODHIP_EINVAL;
  for (int i = 0; i < 2; i++) {
    if (j->dc_quant[i] < 1 || j->dc_quant[i] > kMaxDcQuant) return ODHIP_EINVAL;
  }
  if (j->pic_w < 1 || j->pic_h < 1 || j->pic_w > j->w || j->pic_h > j->h) return ODHIP_EINVAL;
  if (j->plane_split < 0 || j->plane_split > j->nplanes) return ODHIP_EINVAL;
  if (j->px_stride < j->w || j->px_plane_stride < (int64_t)j->px_stride*j->h || (j->px_stride & 3)
   || (j->px_plane_stride & 3)) {
    return ODHIP_EINVAL;
  }
  if (!planes_ok(j->d_px, 4) || !planes_ok(j->d_pred, 4) || !planes_ok(j->d_rec, 4) || !planes_ok(j->d_q, 16)
   || !planes_ok(j->d_tree, 16) || !planes_ok(j->d_dc_rec, 4)) {
    return ODHIP_EINVAL;
  }
  return ODHIP_SUCCESS;
}

#define HAAR_LAUNCH(kernel, grid, s, a) \
  do { \
    if (dec) { \
      if (px16) { \
        if (inter) kernel<5, int16_t, true><<<grid, kNT, 0, s>>>(a); \
        else kernel<5, int16_t, false><<<grid, kNT, 0, s>>>(a); \
      } else { \
        if (inter) kernel<5, uint8_t, true><<<grid, kNT, 0, s>>>(a); \
        else kernel<5, uint8_t, false><<<grid, kNT, 0, s>>>(a); \
      } \
    } else { \
      if (px16) { \
        if (inter) kernel<6, int16_t, true><<<grid, kNT, 0, s>>>(a); \
        else kernel<6, int16_t, false><<<grid, kNT, 0, s>>>(a); \
      } else { \
        if (inter) kernel<6, uint8_t, true><<<grid, kNT, 0, s>>>(a); \
        else kernel<6, uint8_t, false><<<grid, kNT, 0, s>>>(a); \
      } \
    } \
  } while (0)

int haar_run(const odhip_haar_job *j, bool encode, hipStream_t s) {
  const int rc = haar_check(j, encode);
  if (rc) return rc;
  ODHIP_CTX_OR_RETURN(ctx);
  const bool px16 = ctx->fpr != 0;
  if (px16 && (!planes_ok(j->d_px, 8) || !planes_ok(j->d_pred, 8) || !planes_ok(j->d_rec, 8))) return ODHIP_EINVAL;
  const int dec = j->dec;
  const int tile = 64 >> dec;
  const bool inter = j->d_pred != nullptr;
  const size_t nsb = (size_t)(j->w/tile)*(j->h/tile);
  HaarArgs a;
  memset(&a, 0, sizeof(a));
  a.px = j->d_px;
  a.pred = j->d_pred;
  a.rec = j->d_rec;
  a.q = j->d_q;
  a.tree = j->d_tree;
  a.dc_rec = j->d_dc_rec;
  a.px_plane_stride = (long)j->px_plane_stride;
  a.px_stride = j->px_stride;
  a.w = j->w;
  a.h = j->h;
  a.pic_w = j->pic_w;
  a.pic_h = j->pic_h;
  a.plane_split = j->plane_split;
  a.encode = encode;
  if (px16) a.shift = j->lossless ? 4 - (j->depth - 8) : 0;
  else a.shift = j->lossless ? j->depth - 8 : 4;
  for (int d = 0; d < 2; d++) {
    for (int l = 0; l < 6; l++) a.ac[d][l] = make_div(j->quant ? j->quant*kHaarQm[d][l] >> 4 : 1);
    a.dc[d] = make_div(j->dc_quant[d]);
  }
  if (!inter) {
    /* the walk's reconstructions feed the inverse, its symbols need a home beyond the LDS budget */
    HaarState &st = *odhip_ctx_state<HaarState>(ctx, ODHIP_SLOT_HAAR);
    const int rcs = st.dc.grow(2*nsb*(size_t)j->nplanes, s);
    if (rcs) return rcs;
    if (!a.dc_rec) a.dc_rec = st.dc.p;
    a.dc_sym = st.dc.p + nsb*(size_t)j->nplanes;
  }
  const dim3 grid(j->w/tile, j->h/tile, j->nplanes);
  if (encode) HAAR_LAUNCH(k_haar_forward, grid, s, a);
  if (!inter) k_haar_dc<<<j->nplanes, kNT, 0, s>>>(a, tile);
  if (j->d_rec) HAAR_LAUNCH(k_haar_inverse, grid, s, a);
  return odhip_check_launch();
}

}  // namespace

extern "C" int odhip_haar_encode_planes(const odhip_haar_job *job, odhip_stream stream) {
  return haar_run(job, true, (hipStream_t)stream);
}

extern "C" int odhip_haar_decode_planes(const odhip_haar_job *job, odhip_stream stream) {
  return haar_run(job, false, (hipStream_t)stream);
}

extern "C" size_t odhip_haar_sizeof(void) {
  return sizeof(odhip_haar_job);
}

extern "C" int odhip_haar_planes(od_coeff *d_out, const od_coeff *d_in, int nplanes, int w, int h, int ln, int inverse,
 odhip_stream stream) {
  if (!d_out || !d_in || nplanes <= 0 || ln < 2 || ln > 6 || w <= 0 || h <= 0 || w%(1 << ln) || h%(1 << ln)
   || !planes_ok(d_out, 16) || !planes_ok(d_in, 16)) {
    return ODHIP_EINVAL;
  }
  const int n = 1 << ln;
  if (h/n > 65535 || nplanes > 65535) return ODHIP_EINVAL;
  ODHIP_CTX_OR_RETURN(ctx);
  (void)ctx;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(w/n, h/n, nplanes);
  switch (ln) {
    case 2: k_haar_planes<2, 64><<<grid, 64, 0, s>>>(d_out, d_in, w, h, inverse); break;
    case 3: k_haar_planes<3, 64><<<grid, 64, 0, s>>>(d_out, d_in, w, h, inverse); break;
    case 4: k_haar_planes<4, 64><<<grid, 64, 0, s>>>(d_out, d_in, w, h, inverse); break;
    case 5: k_haar_planes<5, kNT><<<grid, kNT, 0, s>>>(d_out, d_in, w, h, inverse); break;
    default: k_haar_planes<6, kNT><<<grid, kNT, 0, s>>>(d_out, d_in, w, h, inverse); break;
  }
  return odhip_check_launch();
}
