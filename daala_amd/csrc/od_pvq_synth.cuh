/* od_pvq_synth.cuh - od_pvq_synthesis_partial (src/pvq.c:1037-1115), stated once for every kernel
   that dequantises: a band's decision (gain, theta, pivot, pulses) back into coefficients.  It scales
   the pulses, undoes the Householder reflection where the band had a reference, and applies the
   inverse quantisation matrix.  Three layers, no global state (tables and planes come in as
   arguments):

     1. per coefficient  od_synth_noref, od_synth_xi, od_synth_ref, in two forms chosen by a policy
                         type (as the transforms choose OdMul24): OdSynthExact, the reference's
                         widths, and OdSynth24, the 24-bit multiplier's;
     2. per band         od_synth_scale, od_synth_theta, od_householder_back: the constants a band
                         needs once;
     3. per chunk        what one lane does with the choice records of a band stage: sixteen coding
                         indices without reference (OdNorefChunk) or a whole 4x4 block in registers
                         (od_noref_leaf4, od_idct4x4_regs), eight positions without reference
                         (od_noref_chunk8) or with one (od_ref_chunk) into a tile or a plane.

   Layers 1 and 2 also compile for the host (with __device__ defined away and a host __mul24 /
   __clz): tests/test_pvq_synth_host.py runs them against the CPU oracle. */
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include "od_pvq_math.cuh"

/* ---- 1. per coefficient ------------------------------------------------------------------------ */

/* OD_MULT16_32_Q16(y, scale) = (int16)y * (int32)scale >> 16 (src/internal.h) without a 32-bit
   multiply: v_mul_hi_i32 and v_mul_lo_u32 issue at a quarter of the rate of the 24-bit multiplier.
   scale = sh*65536 + sl with sh = scale >> 16 (16 bits, signed) and sl = scale & 0xffff, so
   y*scale >> 16 = y*sh + (y*sl >> 16) EXACTLY (y*sh*65536 is a multiple of 65536; |y*sl| < 2^31):
   two 24-bit multiplies of 16-bit operands and a shift.  The value it returns is a QM-scaled
   coefficient of the synthesis, |x| < 2^16 by construction (od_pvq_synthesis_partial scales g so
   that the vector's NORM fits 16 bits, src/pvq.c:1055-1075, and |y_i| <= sqrt(yy)), so the inverse
   quantisation-matrix product x*qm_inv[i] that follows (src/pvq.c:1092) goes through the 24-bit
   multiplier too: the low 32 bits of its 48-bit product are the reference's int product. */
struct OdQ16 {
  int sh;
  int sl;
  __device__ __forceinline__ explicit OdQ16(int scale) : sh(scale >> 16), sl(scale & 0xffff) {}
  __device__ __forceinline__ int mul(int y) const { return __mul24(y, sh) + (__mul24(y, sl) >> 16); }
};
/* pulse j of four packed 16-byte words (eight int16 per pair of words), sign-extended */
__device__ __forceinline__ int od_pulse16(unsigned w, int odd) {
  return odd ? (int)w >> 16 : (int)(w << 16) >> 16;
}

/* The reference's widths: a 64-bit product, OD_SHR_ROUND on 64 bits. */
struct OdSynthExact {
  int32_t scale;
  __device__ __forceinline__ explicit OdSynthExact(int32_t s) : scale(s) {}
  __device__ __forceinline__ int32_t mul(int y) const { return (int32_t)odq_mult16_32_q16(y, scale); }
  __device__ __forceinline__ static int32_t mul_qm(int32_t x, int qmi) { return x*qmi; }
  __device__ __forceinline__ static int32_t shr_round(int32_t x, int s) { return odq_shr_round(x, s); }
};
/* The 24-bit multiplier's (OdQ16 above) and OD_SHR_ROUND in 32 bits: x + the rounding term does not
   overflow for the products of the synthesis (|x*qm_inv| <= 2^31 - 2^15 with a shift of at most 12;
   |r*proj_1| <= 2^30 with one of at most 30). */
struct OdSynth24 {
  OdQ16 q;
  __device__ __forceinline__ explicit OdSynth24(int32_t s) : q(s) {}
  __device__ __forceinline__ int32_t mul(int y) const { return q.mul(y); }
  __device__ __forceinline__ static int32_t mul_qm(int32_t x, int qmi) { return __mul24(x, qmi); }
  __device__ __forceinline__ static int32_t shr_round(int32_t x, int s) { return (x + ((1 << s) >> 1)) >> s; }
};

/* Without reference, src/pvq.c:1081-1092: x = y*scale (Q16, no rounding), out = SHR_ROUND(x*qm_inv, qshift). */
template <class F>
__device__ __forceinline__ int32_t od_synth_noref(const F &f, int y, int qmi, int qshift) {
  return F::shr_round(F::mul_qm(f.mul(y), qmi), qshift);
}

/* With reference, :1094-1114.  Position i of the band holds xm at the Householder pivot m, pulse i
   below it and pulse i - 1 above: y is that pulse. */
template <class F>
__device__ __forceinline__ int16_t od_synth_xi(const F &f, bool is_pivot, int16_t xm, int y) {
  return is_pivot ? xm : (int16_t)f.mul(y);
}
/* ... reflected back through the reference r (ri = r16[i]; proj_1 and outshift from
   od_householder_back) and scaled by the inverse quantisation matrix. */
template <class F>
__device__ __forceinline__ int32_t od_synth_ref(const F &f, bool is_pivot, int16_t xm, int y, int ri, int proj_1,
 int outshift, int qmi, int qshift) {
  const int16_t xi = od_synth_xi(f, is_pivot, xm, y);
  int32_t tmp = odq_mult16_16(ri, proj_1);
  tmp = outshift >= 0 ? F::shr_round(tmp, outshift) : odq_shl32(tmp, -outshift);
  const int16_t v = (int16_t)(xi - tmp);
  return F::shr_round(v*qmi, qshift);
}

/* ---- 2. per band ------------------------------------------------------------------------------- */

/* :1055-1079 from the expanded gain g and yy = <y, y> over the coded pulses. */
struct OdSynthScale {
  int32_t scale;
  int gshift;
  int qshift;
};
__device__ __forceinline__ OdSynthScale od_synth_scale(int32_t g, int32_t yy) {
  OdSynthScale o;
  o.gshift = odq_ilog(g) - 14;
  o.gshift = o.gshift > 0 ? o.gshift : 0;
  o.scale = 0;
  if (yy != 0) {
    int rsqrt_shift;
    const int16_t rsqrt = odq_rsqrt(yy, &rsqrt_shift);
    o.scale = odq_vshr_round(rsqrt*(int64_t)g, rsqrt_shift + o.gshift - 16);
  }
  o.qshift = ODQ_QM_INV_SHIFT - o.gshift;
  return o;
}

/* :1094-1100 for a band with a reference: the pulses' scale times sin(theta), and the pivot's
   coefficient xm = -s*g*cos(theta).  The two double products by 2^-15 are exact.  (od_synth_band is its
   one caller on the device: refb_finish of pvq_refbands.hip writes these two lines out, because through
   this function the decided searches' text changed, profiles/synth_once.txt.  It stays a function of its
   own as the band layer's second step, which the host test runs by itself.) */
struct OdSynthTheta {
  int32_t scale;
  int16_t xm;
};
__device__ __forceinline__ OdSynthTheta od_synth_theta(int32_t scale, int32_t g, int gshift, int32_t theta, int s) {
  OdSynthTheta o;
  o.scale = (int32_t)floor(.5 + (scale*(1./32768))*odq_pvq_sin(theta));
  o.xm = (int16_t)floor(.5 + ((-s*odq_shr_round(g, gshift))*(1./32768))*odq_pvq_cos(theta));
  return o;
}

/* Householder projection constants from l2r = <r, r> and proj = <r, x>, src/pvq.c:573-590. */
struct OdHouseholder {
  int16_t proj_1;
  int outshift;
};
__device__ __forceinline__ OdHouseholder od_householder_back(int32_t l2r, int32_t proj) {
  const int l2r_shift = (odq_ilog(l2r) - 1) - 14;
  const int16_t l2r_norm = (int16_t)odq_vshr_round(l2r, l2r_shift);
  const int16_t rcp = odq_rcp(l2r_norm);
  const int proj_shift = (odq_ilog(abs(proj)) - 1) - 14;
  const int16_t proj_norm = (int16_t)odq_vshr_round(proj, proj_shift);
  OdHouseholder o;
  o.proj_1 = (int16_t)odq_mult16_16_q15(proj_norm, rcp);
  const int os = 14 - proj_shift - 1 + l2r_shift;
  o.outshift = os > 30 ? 30 : os;
  return o;
}

/* A whole band in one lane through accessors, given g, yy = <y, y>, theta and the pivot (m, s): R16(i)
   the QM-scaled reference after od_compute_householder, Y(i) the pulses, OUT(i, v) writes coefficient
   i (it may overwrite what R16(i) reads: every loop reads position i before it writes it).  x = [y*scale
   with xm inserted at m]; Householder back; inverse QM.  Two passes over the band recompute x[i]
   instead of holding 128 values. */
template <class F, class R16At, class YAt, class OutAt>
__device__ __forceinline__ void od_synth_band(R16At R16, YAt Y, OutAt OUT, int n, int noref, int32_t g, int32_t yy,
 int32_t theta, int m, int s, const int16_t *qm_inv) {
  const OdSynthScale sy = od_synth_scale(g, yy);
  if (noref) {
    const F f(sy.scale);
    for (int i = 0; i < n; i++) OUT(i, od_synth_noref(f, Y(i), qm_inv[i], sy.qshift));
    return;
  }
  const OdSynthTheta th = od_synth_theta(sy.scale, g, sy.gshift, theta, s);
  const F f(th.scale);
  int32_t l2r = 0;
  int32_t proj = 0;
  /* the pulse under position i: none at the pivot, where Y is not read (Y(-1) would lie before the band for m = 0) */
  auto pulse = [&](int i) { return i == m ? 0 : (int)Y(i < m ? i : i - 1); };
  for (int i = 0; i < n; i++) {
    const int ri = R16(i);
    l2r += odq_mult16_16(ri, ri);
    proj += odq_mult16_16(ri, od_synth_xi(f, i == m, th.xm, pulse(i)));
  }
  const OdHouseholder hb = od_householder_back(l2r, proj);
  for (int i = 0; i < n; i++) {
    OUT(i, od_synth_ref(f, i == m, th.xm, pulse(i), R16(i), hb.proj_1, hb.outshift, qm_inv[i], sy.qshift));
  }
}

/* ---- 3. per chunk ------------------------------------------------------------------------------ */
#ifdef __HIPCC__
#include <type_traits>
#include "../../include/daala_hip.h"
#include "od_lift.cuh"
#include "gen/od_scan_tables.h"

/* Compile-time loop: f(std::integral_constant<int, J>) for J in [J0, J1) (register arrays indexed with
   scan-table entries stay in registers only when the indices are constant expressions). */
template <int J0, int J1, class Fn>
__device__ __forceinline__ void od_static_for(Fn &&f) {
  if constexpr (J0 < J1) {
    f(std::integral_constant<int, J0>{});
    od_static_for<J0 + 1, J1>(f);
  }
}

/* Sixteen consecutive coding indices j0 .. j0 + 15 of one block, no-reference band stage (choice
   record: slot, coded, scale, qshift): everything the chunk needs comes straight from global memory
   into registers, in one dependent chain band -> record -> pulses with the table loads beside it.
   A chunk touches at most two bands (coding indices 16..31 hold two bands of 8). */
struct OdNorefChunk {
  /* Plain state, open to the kernel that holds the chunk: the walking kernels (WalkPvq) issue heads() one
     group ahead and pulses() later, so they clear chs / dc and yq by halves, each in front of its own load
     phase, and their 4x4 form reads the records and pulses straight from here. */
  int4 chs[2];
  int4 yq[2];
  int dc;
  __device__ __forceinline__ void clear() {
    chs[0] = chs[1] = make_int4(0, 0, 0, 0);
    yq[0] = yq[1] = make_int4(0, 0, 0, 0);
    dc = 0;
  }
  /* the records of the bands of its two halves (ONE: a 4x4 block has a single band) and, for the
     chunk at 0, the DC, which is passed through */
  template <bool ONE = false>
  __device__ __forceinline__ void heads(const int4 *rec, int bnd0, int bnd1, const od_coeff *dc_at, int j0) {
    if (j0 == 0) dc = *dc_at;
    chs[0] = rec[bnd0];
    if constexpr (ONE) chs[1] = chs[0];
    else chs[1] = rec[bnd1];
  }
  /* ... and, once those records are here, the chosen pulse vectors (those of a band that codes
     nothing are not read: zero in, zero out, and (0 + rnd) >> qshift == 0) */
  __device__ __forceinline__ void pulses(const int16_t *y, unsigned nblocks, unsigned blk, int lsh, int j0) {
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
      if (chs[hf].y != 0) {
        yq[hf] = *reinterpret_cast<const int4 *>(y + (((unsigned)chs[hf].x*nblocks + blk) << lsh) + j0 + 8*hf);
      }
    }
  }
  /* registers -> the block at ts of a tile of pitch P: the scatter to raster through the packed scan
     table (y << 8 | x of coding index j; od_coding_order_to_raster, src/partition.c:176-194) */
  template <int P>
  __device__ __forceinline__ void commit(int *ts, const int4 (&qm4)[2], const int4 (&sc4)[2], int j0) const {
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
      const int yd[4] = {yq[hf].x, yq[hf].y, yq[hf].z, yq[hf].w};
      const int qd[4] = {qm4[hf].x, qm4[hf].y, qm4[hf].z, qm4[hf].w};
      const int sd[4] = {sc4[hf].x, sc4[hf].y, sc4[hf].z, sc4[hf].w};
      const int4 ch = chs[hf];
      const OdSynth24 f(ch.z);
#pragma unroll
      for (int e = 0; e < 4; e++) {
#pragma unroll
        for (int u = 0; u < 2; u++) {
          const int yv = od_pulse16((unsigned)yd[e], u);
          const int qmi = u ? qd[e] >> 16 : (int)(short)qd[e];
          const int xy = u ? (unsigned)sd[e] >> 16 : sd[e] & 0xffff;
          int v = od_synth_noref(f, yv, qmi, ch.w);
          if (hf == 0 && e == 0 && u == 0 && j0 == 0) v = dc;
          ts[(xy >> 8)*P + (xy & 255)] = v;
        }
      }
    }
  }
};
/* the chunk's inverse-QM entries and scan positions */
__device__ __forceinline__ void od_noref_tables(int4 (&qm4)[2], int4 (&sc4)[2], const int16_t *qm_inv,
 const unsigned short *scan, int j0) {
#pragma unroll
  for (int hf = 0; hf < 2; hf++) {
    qm4[hf] = *reinterpret_cast<const int4 *>(qm_inv + j0 + 8*hf);
    sc4[hf] = *reinterpret_cast<const int4 *>(scan + j0 + 8*hf);
  }
}

/* A 4x4 block is ONE band of 15 coefficients plus its DC.  Coding positions 1..15 dequantised
   straight into a 4x4 register array (the scan is a compile-time constant: no scan table, no
   scatter through LDS, the inverse quantisation matrix in scalar registers). */
__device__ __forceinline__ void od_noref_leaf4(int (&m)[4][4], int32_t scale, int qshift, const unsigned (&yw)[8],
 const int16_t *qm_inv) {
  const OdSynth24 f(scale);
  od_static_for<1, 16>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    m[OD_SCAN_XY[j][1]][OD_SCAN_XY[j][0]] = od_synth_noref(f, od_pulse16(yw[j >> 1], j & 1), (int)qm_inv[j], qshift);
  });
}

/* od_bin_idct4x4 (rows, then columns, src/dct.c:158-163) in registers, the four rows of the block
   written into the tile as 16-byte pieces. */
template <int P>
__device__ __forceinline__ void od_idct4x4_regs(int *ts, const int (&m)[4][4]) {
  using T = OdMul24;
  T q[4][4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const T in[4] = {T(m[r][0]), T(m[r][1]), T(m[r][2]), T(m[r][3])};
    od_idct_lift<0>(q[r], in);
  }
  T o[4][4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const T in[4] = {q[0][c], q[1][c], q[2][c], q[3][c]};
    T out[4];
    od_idct_lift<0>(out, in);
    o[0][c] = out[0];
    o[1][c] = out[1];
    o[2][c] = out[2];
    o[3][c] = out[3];
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    *reinterpret_cast<int4 *>(ts + r*P) = make_int4(o[r][0], o[r][1], o[r][2], o[r][3]);
  }
}

/* Where a chunk of eight positions goes: position (y, x) of its block in a tile of pitch P, or in a
   raster plane of width w. */
template <int P>
struct OdTileSink {
  int *t;
  __device__ __forceinline__ void put(int y, int x, int v) const { t[y*P + x] = v; }
};
struct OdPlaneSink {
  od_coeff *p;
  int w;
  __device__ __forceinline__ void put(int y, int x, int v) const { p[(long)y*w + x] = v; }
};

/* Eight consecutive coding positions of one band, without reference: put(e, value) for e = 0..7
   from 16 bytes of pulses and 16 of inverse-QM entries. */
template <class F, class Put>
__device__ __forceinline__ void od_noref_chunk8(const F &f, int qshift, const unsigned (&yw)[4],
 const unsigned (&qw)[4], Put put) {
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const int yv = od_pulse16(yw[e >> 1], e & 1);
    const int qmi = (int16_t)(qw[e >> 1] >> (16*(e & 1)));
    put(e, od_synth_noref(f, yv, qmi, qshift));
  }
}

/* Eight consecutive coding positions c0 .. c0 + 7 of block blk from a with-reference band stage's
   choice (the per-coefficient part of od_pvq_synthesis_partial, src/pvq.c:1081-1114, and the bands
   that were skipped): a chunk never straddles a band (bands start at 1, 16, 24, 32, 64, ...; the
   chunk at 0 holds the DC, which is passed through, and the first seven coefficients of band 0).
   rec: the band's four records, [2] = {mode, slot, scale, qshift}, [3] = {xm, m, proj_1, outshift};
   mode 0 zero, 1 / 4 the reference / its negative, 2 without reference, 3 with.  off: the band's
   first coding position (the caller knows the leaf level, at run time or at compile time); coef0 /
   ref0: the block's corner in the coefficient and reference planes of width w.  Pulses, reference,
   inverse QM and scan positions are 16-byte loads. */
template <class F, class Sink>
__device__ __forceinline__ void od_ref_chunk(const Sink &sink, const int4 *rec, int c0, int off, int len, long blk,
 long nblocks, const od_coeff *coef0, const od_coeff *ref0, int w, const int16_t *y, const int16_t *r16,
 const int16_t *qm_inv, const unsigned short *scan) {
  const int4 ca = rec[2];
  const int mode = ca.x;
  const uint4 sc4 = *reinterpret_cast<const uint4 *>(scan + c0);
  const unsigned scw[4] = {sc4.x, sc4.y, sc4.z, sc4.w};
  int py[8];
  int px[8];
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const unsigned pk = (scw[e >> 1] >> (16*(e & 1))) & 0xffffu;
    py[e] = (int)(pk >> 8);
    px[e] = (int)(pk & 255);
  }
  const bool first = c0 == 0;
  if (first) sink.put(0, 0, *coef0);        /* the DC sits at (0, 0) */
  if (mode == 0) {
#pragma unroll
    for (int e = 0; e < 8; e++) if (!(first && e == 0)) sink.put(py[e], px[e], 0);
    return;
  }
  if (mode == 1 || mode == 4) {
#pragma unroll
    for (int e = 0; e < 8; e++) {
      if (first && e == 0) continue;
      const od_coeff rv = ref0[(long)py[e]*w + px[e]];
      sink.put(py[e], px[e], mode == 4 ? -rv : rv);
    }
    return;
  }
  const int yslot = ca.y;
  const int qshift = ca.w;
  const uint4 q4 = *reinterpret_cast<const uint4 *>(qm_inv + c0);
  const unsigned qw[4] = {q4.x, q4.y, q4.z, q4.w};
  unsigned yw[4] = {0, 0, 0, 0};
  int yprev = 0;                             /* pulse just before the chunk */
  if (yslot >= 0) {
    const int16_t *yp = y + ((long)yslot*nblocks + blk)*len + c0;
    const uint4 y4 = *reinterpret_cast<const uint4 *>(yp);
    yw[0] = y4.x;
    yw[1] = y4.y;
    yw[2] = y4.z;
    yw[3] = y4.w;
    if (mode == 3 && c0 > off) yprev = yp[-1];
  }
  const F f(ca.z);
  if (mode == 2) {
    od_noref_chunk8(f, qshift, yw, qw, [&](int e, int v) {
      if (!(first && e == 0)) sink.put(py[e], px[e], v);
    });
    return;
  }
  const int4 cb = rec[3];
  const int m = cb.y;
  const uint4 r4 = *reinterpret_cast<const uint4 *>(r16 + blk*len + c0);
  const unsigned rw[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
  for (int e = 0; e < 8; e++) {
    if (first && e == 0) continue;
    const int i = c0 + e - off;              /* position inside the band */
    const int yv = od_pulse16(yw[e >> 1], e & 1);
    const int ym1 = e == 0 ? yprev : od_pulse16(yw[(e - 1) >> 1], (e - 1) & 1);
    const int qmi = (int16_t)(qw[e >> 1] >> (16*(e & 1)));
    const int ri = (int16_t)(rw[e >> 1] >> (16*(e & 1)));
    sink.put(py[e], px[e], od_synth_ref(f, i == m, (int16_t)cb.x, i < m ? yv : ym1, ri, cb.z, cb.w, qmi, qshift));
  }
}
#endif
