"""od_pvq_synth.cuh (the one statement of od_pvq_synthesis_partial every dequantising kernel calls) compiled for the
HOST: its per-coefficient layer form against form - the 24-bit multiplier's against the reference's widths - and its
per-coefficient and per-band layers against the CPU oracle's od_pvq_synthesis_partial, bit for bit.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <stdint.h>
#include <math.h>
#include <stdlib.h>
#define __device__
#define __host__
#define __forceinline__ inline
/* v_mul_i32_i24: the low 32 bits of the product of the operands' sign-extended low 24 bits */
static inline int sext24(int a) { return (int)((unsigned)a << 8) >> 8; }
static inline int __mul24(int a, int b) { return (int)(int64_t)((int64_t)sext24(a)*sext24(b)); }
static inline int __clz(int x) { return x ? __builtin_clz((unsigned)x) : 32; }
static inline double __ddiv_rn(double a, double b) { return a/b; }
#include "od_pvq_synth.cuh"

/* OdQ16::mul against the 64-bit product for every int16 y: the number of mismatches */
extern "C" long q16_mismatches(const int32_t *scales, int ns) {
  long bad = 0;
  for (int k = 0; k < ns; k++) {
    const OdQ16 q(scales[k]);
    for (int y = -32768; y < 32768; y++) bad += q.mul(y) != (int32_t)((int64_t)y*scales[k] >> 16);
  }
  return bad;
}

/* od_synth_noref, 24-bit form against exact form, for every int16 y with |y*scale >> 16| < 2^16 */
extern "C" long noref_mismatches(const int32_t *scales, int ns, const int16_t *qmi, int nq, long *compared) {
  long bad = 0;
  long cnt = 0;
  for (int k = 0; k < ns; k++) {
    const OdSynthExact fe(scales[k]);
    const OdSynth24 f24(scales[k]);
    for (int y = -32768; y < 32768; y++) {
      const int64_t x = (int64_t)y*scales[k] >> 16;
      if (x <= -65536 || x >= 65536) continue;
      for (int j = 0; j < nq; j++) {
        for (int qshift = 0; qshift <= 12; qshift += 4) {
          bad += od_synth_noref(f24, y, qmi[j], qshift) != od_synth_noref(fe, y, qmi[j], qshift);
          cnt++;
        }
      }
    }
  }
  *compared = cnt;
  return bad;
}

/* the 32-bit rounding shift against odq_shr_round, s = 0..30, wherever x + the rounding term fits 32 bits */
extern "C" long shr_mismatches(const int32_t *x, int nx, long *compared) {
  long bad = 0;
  long cnt = 0;
  for (int s = 0; s <= 30; s++) {
    for (int i = 0; i < nx; i++) {
      if ((int64_t)x[i] + ((1 << s) >> 1) > INT32_MAX) continue;
      bad += OdSynth24::shr_round(x[i], s) != odq_shr_round(x[i], s) || OdSynthExact::shr_round(x[i], s) != odq_shr_round(x[i], s);
      cnt++;
    }
  }
  *compared = cnt;
  return bad;
}

/* a band through layers 1 and 2, as k_synthesis runs it; every index the accessors are asked for is checked: the
   band has n reference and output positions and n - !noref pulses */
static long g_bad_index = 0;
extern "C" long bad_indices(void) { return g_bad_index; }
template <class F>
static void band(int32_t *out, const int32_t *y, const int16_t *r16, int n, int noref, int32_t g, int32_t theta, int m,
 int s, const int16_t *qm_inv) {
  const int ny = n - !noref;
  int yy = 0;
  for (int i = 0; i < ny; i++) yy += y[i]*y[i];
  od_synth_band<F>([&](int i) { if (i < 0 || i >= n) { g_bad_index++; return 0; } return (int)r16[i]; },
   [&](int i) { if (i < 0 || i >= ny) { g_bad_index++; return 0; } return (int)y[i]; },
   [&](int i, int v) { if (i < 0 || i >= n) g_bad_index++; else out[i] = v; },
   n, noref, g, yy, theta, m, s, qm_inv);
}
/* the Householder shift of a band with a reference, from the same layers */
extern "C" int band_outshift(const int32_t *y, const int16_t *r16, int n, int32_t g, int32_t theta, int m, int s) {
  int yy = 0;
  for (int i = 0; i < n - 1; i++) yy += y[i]*y[i];
  const OdSynthScale sy = od_synth_scale(g, yy);
  const OdSynthTheta th = od_synth_theta(sy.scale, g, sy.gshift, theta, s);
  const OdSynthExact f(th.scale);
  int32_t l2r = 0;
  int32_t proj = 0;
  for (int i = 0; i < n; i++) {
    l2r += odq_mult16_16(r16[i], r16[i]);
    proj += odq_mult16_16(r16[i], od_synth_xi(f, i == m, th.xm, i == m ? 0 : y[i < m ? i : i - 1]));
  }
  return od_householder_back(l2r, proj).outshift;
}
extern "C" void band_exact(int32_t *out, const int32_t *y, const int16_t *r16, int n, int noref, int32_t g, int32_t theta,
 int m, int s, const int16_t *qm_inv) {
  band<OdSynthExact>(out, y, r16, n, noref, g, theta, m, s, qm_inv);
}
extern "C" void band_24(int32_t *out, const int32_t *y, const int16_t *r16, int n, int noref, int32_t g, int32_t theta,
 int m, int s, const int16_t *qm_inv) {
  band<OdSynth24>(out, y, r16, n, noref, g, theta, m, s, qm_inv);
}
extern "C" int band_gshift(int32_t g) { return od_synth_scale(g, 1).gshift; }
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("synth")
    # the header's own includes ask for the HIP runtime; on the host the few intrinsics it uses are the ones above
    os.makedirs(d / "hip")
    (d / "hip" / "hip_runtime.h").write_text("")
    src = d / "synth.cc"
    src.write_text(SRC)
    so = d / "libsynth.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fwrapv", "-ffp-contract=off", "-I", str(d),
                    "-I", os.path.join(ROOT, "daala_amd", "csrc"), "-o", str(so), str(src)], check=True, capture_output=True)
    L = ctypes.CDLL(str(so))
    for f in (L.q16_mismatches, L.noref_mismatches, L.shr_mismatches, L.bad_indices):
        f.restype = ctypes.c_long
    return L


EDGE_SCALES = [0, 1, -1, 65535, -65535, 65536, -65536, -2 ** 31, 2 ** 31 - 1]


def test_q16_multiply_equals_the_64_bit_product_for_every_pulse(lib):
    from _libs import P
    rng = np.random.RandomState(11)
    scales = np.concatenate([np.array(EDGE_SCALES, np.int64), rng.randint(-2 ** 31, 2 ** 31, size=2000),
                             rng.randint(-2 ** 17, 2 ** 17, size=1000)]).astype(np.int32)
    assert lib.q16_mismatches(P(scales), len(scales)) == 0


def test_24_bit_noref_equals_the_exact_form_on_the_synthesis_domain(lib):
    """The domain the header's comment claims: |y*scale >> 16| < 2^16 (a QM-scaled coefficient of the synthesis),
    any int16 inverse-QM entry, qshift 0..12.  Scales around +-2^16 and +-2^17 put |x| at the domain's edges
    (|y| up to 2^15 times a scale of 2^17 is 2^16), the largest ones leave only the smallest pulses inside."""
    from _libs import P
    rng = np.random.RandomState(12)
    scales = np.concatenate([np.array(EDGE_SCALES, np.int64),
                             np.array([2 ** 17, -2 ** 17, 2 ** 17 - 1, 2 ** 17 + 1, 131071 * 2, 2 ** 24, -2 ** 24], np.int64),
                             rng.randint(-2 ** 18, 2 ** 18, size=60), rng.randint(-2 ** 31, 2 ** 31, size=20)]).astype(np.int32)
    qmi = np.array([-32768, -1, 0, 1, 16, 4096, 4097, 21845, 32767], np.int16)
    compared = ctypes.c_long(0)
    bad = lib.noref_mismatches(P(scales), len(scales), P(qmi), len(qmi), ctypes.byref(compared))
    assert compared.value > 10 ** 7
    assert bad == 0


def test_32_bit_rounding_shift_equals_od_shr_round(lib):
    from _libs import P
    rng = np.random.RandomState(13)
    x = np.concatenate([np.array([0, 1, -1, 2 ** 30, -2 ** 30, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 2 ** 15, 2 ** 31 - 2 ** 11 - 1,
                                  2 ** 30 + 2 ** 29 - 1], np.int64),
                        2 ** np.arange(31, dtype=np.int64) - 1, -(2 ** np.arange(31, dtype=np.int64)),
                        rng.randint(-2 ** 31, 2 ** 31, size=200000)]).astype(np.int32)
    compared = ctypes.c_long(0)
    assert lib.shr_mismatches(P(x), len(x), ctypes.byref(compared)) == 0
    assert compared.value > 31 * 100000


def _bands(rng, n, noref):
    """Pulse vectors: none (yy == 0), one pulse, few, many."""
    ys = []
    for k in (0, 1, 3, 17, 60):
        y = np.zeros(n, np.int32)
        for _ in range(k):
            y[rng.randint(n - (not noref))] += rng.choice([-1, 1])
        ys.append(y)
    return ys


@pytest.mark.parametrize("n", [8, 15, 32, 128])
def test_band_synthesis_equals_the_oracle(lib, n):
    """Both forms of layer 1 under layer 2's constants against odo_pvq_synthesis_partial: the pivot m at every position,
    both signs, theta at 0, at its maximum (2^15: pi/2) and between, no pulses at all, gains on both sides of 2^14
    (gshift > 0 above) and gains of 1 and 3 (a projection of a few units on a long reference: the Householder
    shift reaches its clamp of 30), without and with reference."""
    from _libs import P, oracle
    o = oracle()
    rng = np.random.RandomState(20 + n)
    gains = [0, 1, 3, 300, 16383, 16384, 70000, 900000]
    assert [lib.band_gshift(g) for g in gains] == [0, 0, 0, 0, 0, 1, 3, 6]
    checked = 0
    outshifts = {}
    for trial, g in enumerate(gains):
        qmi = rng.randint(16, 32768, size=n).astype(np.int16)
        v = rng.laplace(size=n)
        v /= np.sqrt((v * v).sum())
        # a reference as pvq_theta scales it: the vector's norm fits 15 bits, so sum r^2 stays below 2^31
        r16 = np.round(v * [300, 5000, 16000, 30000][trial % 4]).astype(np.int16)
        for noref in (0, 1):
            for y in _bands(rng, n, noref):
                for m in (range(n) if not noref else [0]):
                    for s in ((-1, 1) if not noref else [1]):
                        for theta in ((0, 32768, int(rng.randint(1, 32768))) if not noref else [0]):
                            want = np.zeros(n, np.int32)
                            o.odo_pvq_synthesis_partial(P(want), P(y), P(r16), n, noref, g, theta, m, s, P(qmi))
                            for fn in (lib.band_exact, lib.band_24):
                                got = np.full(n, 0x55555555, np.int32)
                                fn(P(got), P(y), P(r16), n, noref, g, theta, m, s, P(qmi))
                                assert np.array_equal(got, want), (n, g, noref, m, s, theta)
                            if not noref:
                                outshifts.setdefault(g, set()).add(lib.band_outshift(P(y), P(r16), n, g, theta, m, s))
                            checked += 1
    assert checked >= len(gains) * 5 * (6 * n + 1)
    # no accessor was asked for a position outside its band (the pivot at 0 must not read pulse -1)
    assert lib.bad_indices() == 0
    # the Householder shift reaches its clamp under the tiny gains, and both sides of the clamp are taken
    assert 30 in outshifts[1] | outshifts[3], outshifts
    assert min(min(v) for v in outshifts.values()) < 30, outshifts
