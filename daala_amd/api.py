"""ctypes binding of libdaalahip.so + torch-tensor convenience wrappers.

Names and argument meaning mirror the C ABI (include/daala_hip.h), which in
turn mirrors the reference's surfaces for this path (od_dct_func_2d,
od_*filter*_split / _frame_sbs, pvq_search_rdo_double).
"""
import ctypes
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class DaalaHipError(RuntimeError):
    pass


# Every struct and every integer #define of include/daala_hip.h, as the header lays them out (daala_amd/_abi.py).  A
# pointer field is a c_void_p and keeps nothing alive: whoever builds a struct owns what it points to across the call.
_S, _C = _abi.structs(), _abi.constants()


def _defines(*names):
    """The values of ODHIP_<name> for each of names."""
    return tuple(_C["ODHIP_" + n] for n in names)


# odhip_*_sizeof(index) of the loaded library against the struct it has to agree with
_LAYOUT_GUARD = {("odhip_me_sizeof", 0): "odhip_me_job", ("odhip_me_sizeof", 1): "odhip_me_cand",
                 ("odhip_me_sizeof", 2): "odhip_me_job2", ("odhip_me_sizeof", 4): "odhip_me_job3",
                 ("odhip_me_sizeof", 5): "odhip_me_job4", ("odhip_mc_sizeof", 0): "odhip_mv_point",
                 ("odhip_mc_sizeof", 1): "odhip_mc_job", ("odhip_haar_sizeof", None): "odhip_haar_job"}


def _check_layouts(L):
    """Raise when the library was compiled against another layout of a struct than the header's."""
    for (fn, index), name in _LAYOUT_GUARD.items():
        got, want = getattr(L, fn)(*(() if index is None else (index,))), ctypes.sizeof(_S[name])
        if got != want:
            raise DaalaHipError("%s is %d bytes in %s and %d bytes in include/daala_hip.h: rebuild the library"
                                % (name, got, lib_path(), want))
    return L


# The experiments build (-DODHIP_EXPERIMENTS: superseded kernel generations and ablations behind
# their ODHIP_* switches; daala_amd/build.py): ODHIP_LIB=EXPERIMENTS_LIB selects it for a process.
EXPERIMENTS_LIB = os.path.join(_HERE, "lib", "libdaalahip_exp.so")


def lib_path():
    # ODHIP_LIB: another build of the same library (kernel A/B experiments, tools/)
    return os.environ.get("ODHIP_LIB") or os.path.join(_HERE, "lib", "libdaalahip.so")


def lib():
    """The loaded C-ABI library.  Fails loudly when it is missing."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise DaalaHipError(
                "%s not built: run `python -m daala_amd.build` "
                "(there is no CPU fallback)" % path)
        # PyTorch-ROCm ships its own copy of the HIP runtime; when it is going to be used in
        # this process (device tensors, streams) it has to be the one the process binds
        # first - the library loaded first would otherwise bring /opt/rocm's copy and
        # torch.cuda then finds no device.  A pure-C consumer never gets here.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _LIB = _check_layouts(_abi.bind(ctypes.CDLL(path)))     # prototypes from the header, layouts against it
    return _LIB


# ERANGE: a band needs more pulses than ODHIP_PVQ_MAX_K; EBUSY: the export ring slot of the next step is still held
ERANGE, EBUSY = _defines("ERANGE", "EBUSY")


class PulseRangeError(DaalaHipError):
    """A band's reference candidate has more than 32767 pulses (quantiser too fine for the int16 pulse vectors): the
    results are NOT the reference's."""


class ExportRingBusyError(DaalaHipError):
    """odhip_pipe_step found the export ring slot of its step still held (ODHIP_EBUSY): nothing was enqueued; release
    a taken step (Pipe.export_release) and step again."""


def _check(rc, what):
    if rc == EBUSY:
        raise ExportRingBusyError("%s: the export ring slot of the next step is still held (release a step first), "
                                  "or its metrics slot (take a step first)" % what)
    if rc == ERANGE:
        raise PulseRangeError("%s: a band needs more pulses than ODHIP_PVQ_MAX_K = 32767; the results since the last "
                              "sync are not the reference's" % what)
    if rc != 0:
        raise DaalaHipError("%s failed with code %d" % (what, rc))


def pvq_k_range_take():
    """(no-reference bands, with-reference bands) whose candidate exceeded ODHIP_PVQ_MAX_K since the last call; cleared.
    Synchronise the stream of the band stage first."""
    a = ctypes.c_uint()
    b = ctypes.c_uint()
    rc = lib().odhip_pvq_k_range_take(ctypes.byref(a), ctypes.byref(b))
    if rc not in (0, ERANGE):
        _check(rc, "odhip_pvq_k_range_take")
    return a.value, b.value


def init(device=0):
    _check(lib().odhip_init(int(device)), "odhip_init")


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _need(t, dtype, what):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype
            and t.is_contiguous()):
        raise DaalaHipError("%s must be a contiguous CUDA tensor of %s" % (what, dtype))


# ---- batched transforms ---------------------------------------------------
def _dct_batch(fn, ln, x, exact32, out):
    import torch
    n = 4 << ln
    _need(x, torch.int32, "x")
    if x.shape[-2:] != (n, n):
        raise DaalaHipError("x must be [..., %d, %d]" % (n, n))
    nblocks = x.numel() // (n * n)
    if out is None:
        out = torch.empty_like(x)
    _check(fn(int(ln), _p(out), _p(x), nblocks, int(bool(exact32)), _stream()), fn.__name__)
    return out


def fdct2d_batch(ln, x, exact32=False, out=None):
    """od_bin_fdctNxN (N = 4 << ln) of every [N, N] tile of x (int32, CUDA)."""
    return _dct_batch(lib().odhip_fdct2d_batch, ln, x, exact32, out)


def idct2d_batch(ln, y, exact32=False, out=None):
    return _dct_batch(lib().odhip_idct2d_batch, ln, y, exact32, out)


def _dct_plane(fn, ln, x, exact32):
    import torch
    _need(x, torch.int32, "plane")
    h, w = x.shape
    out = torch.empty_like(x)
    _check(fn(int(ln), _p(out), w, _p(x), w, w, h, int(bool(exact32)), _stream()),
           fn.__name__)
    return out


def fdct2d_plane(ln, x, exact32=False):
    return _dct_plane(lib().odhip_fdct2d_plane, ln, x, exact32)


def idct2d_plane(ln, y, exact32=False):
    return _dct_plane(lib().odhip_idct2d_plane, ln, y, exact32)


def filter_batch(f, x, inverse=False, out=None):
    """(4 << f)-tap lapping filter (od_pre_filterN / od_post_filterN) of every row
    of x: int32 [count, 4 << f] CUDA."""
    import torch
    _need(x, torch.int32, "x")
    count, n = x.shape
    if n != 4 << f:
        raise DaalaHipError("x must be [count, %d]" % (4 << f))
    if out is None:
        out = torch.empty_like(x)
    _check(lib().odhip_filter_batch(int(f), int(bool(inverse)), _p(out), _p(x), count, _stream()), "odhip_filter_batch")
    return out


def dering_planes(x, xdec, dirs, pli, bskip, thresholds, overlap=1, coeff_shift=4):
    """od_dering on every superblock of every plane for every candidate threshold.
    x int16 [nplanes, h, w]; dirs int32 [nplanes, h/(8>>xdec)... see daala_hip.h] =
    [nplanes, nvsb*8, nhsb*8]; bskip uint8 [nplanes, rows, skip_stride];
    thresholds int32 [nplanes, ncand, nvsb*nhsb].  Returns y int16
    [nplanes, ncand, h, w]."""
    import torch
    _need(x, torch.int16, "x")
    _need(dirs, torch.int32, "dirs")
    _need(bskip, torch.uint8, "bskip")
    _need(thresholds, torch.int32, "thresholds")
    nplanes, h, w = x.shape
    n = 64 >> xdec
    nhsb, nvsb = w // n, h // n
    ncand = thresholds.shape[1]
    y = torch.empty((nplanes, ncand, h, w), dtype=torch.int16, device=x.device)
    _check(lib().odhip_dering_planes(_p(y), _p(x), w, nhsb, nvsb, int(xdec), nplanes, _p(dirs), int(pli), _p(bskip),
                                     bskip.shape[2], bskip.shape[1] * bskip.shape[2], _p(thresholds), ncand,
                                     int(overlap), int(coeff_shift), _stream()), "odhip_dering_planes")
    return y


# ---- fused lapped stage -----------------------------------------------------
def px_dtype():
    """torch dtype of picture planes in the calling thread's current context: uint8, or int16
    samples at 12 bits when the context is in full-precision-references mode
    (Context.set_fpr, odhip_ctx_set_fpr)."""
    import torch
    L = lib()
    cur = L.odhip_get_current()
    return torch.int16 if cur and L.odhip_ctx_get_fpr(cur) == 1 else torch.uint8


def forward_pyramid(px, dec, pic_w, pic_h, levels=None, want=None):
    """px: uint8 (int16 in a full-precision-references context) [nplanes, h, w] CUDA.
    Returns a list of int32 [nplanes, h, w] tensors, index bs = 0..4-dec (None where
    `want` excludes a level)."""
    import torch
    _need(px, px_dtype(), "px")
    nplanes, h, w = px.shape
    top = 4 - dec
    if levels is None:
        # ONE allocation, the planes a non-power-of-two distance apart: separate torch allocations
        # of 127.5 MiB (16 frames of 1080p) land exactly 128 MiB apart, and five streams written
        # concurrently at addresses equal modulo 2^27 share HBM channels and banks - 216 us per
        # launch instead of 173 (tools/pyr_skew.py, DESIGN.md par. 4)
        n = nplanes * h * w
        stride = ((n + 1023) & ~1023) + (68 << 10)          # int32 elements; +272 KiB
        ks = [bs for bs in range(top + 1) if (want is None or bs in want)]
        levels = [None] * (top + 1)
        if len(ks) == 1:
            # a single level: its own allocation (a view of a shared block would pin the whole
            # block for as long as the caller keeps that one level)
            levels[ks[0]] = torch.empty((nplanes, h, w), dtype=torch.int32, device=px.device)
        else:
            big = torch.empty((max(len(ks), 1) * stride,), dtype=torch.int32, device=px.device)
            for i, bs in enumerate(ks):
                levels[bs] = big[i * stride: i * stride + n].view(nplanes, h, w)
    arr = (ctypes.c_void_p * 5)()
    for bs in range(5):
        t = levels[bs] if bs <= top else None
        arr[bs] = ctypes.c_void_p(t.data_ptr() if t is not None else None)
    _check(lib().odhip_forward_pyramid(arr, _p(px), w, h * w, nplanes, w, h, int(dec), int(pic_w), int(pic_h),
                                       _stream()), "odhip_forward_pyramid")
    return levels


def inverse_level(coef, dec, leaf_bs, pic_w, pic_h, out=None):
    """coef: int32 [nplanes, h, w] at uniform partition level leaf_bs ->
    uint8 [nplanes, h, w] reconstructed pixels."""
    import torch
    _need(coef, torch.int32, "coef")
    nplanes, h, w = coef.shape
    if out is None:
        out = torch.empty((nplanes, h, w), dtype=px_dtype(), device=coef.device)
    _check(lib().odhip_inverse_level(_p(out), w, h * w, _p(coef), nplanes, w, h, int(dec), int(leaf_bs), int(pic_w),
                                     int(pic_h), _stream()), "odhip_inverse_level")
    return out


def forward_partition(px, bmap, dec, pic_w, pic_h, planes_per_frame=1, out=None):
    """The coefficients the encoder codes at each frame's own block-size map (odhip_forward_partition).
    px: uint8 (int16 in a full-precision-references context) [nplanes, h, w] CUDA; bmap: uint8
    [nplanes / planes_per_frame, (h << dec) / 8, (w << dec) / 8] CUDA (or one [rows, cols] map for every
    plane), one entry per 8x8 luma area, 0 = four 4x4 blocks ... 4 = 64x64.  Returns int32 [nplanes, h, w]:
    every leaf's forward DCT where it lies."""
    import torch
    _need(px, px_dtype(), "px")
    nplanes, h, w = px.shape
    bmap, planes_per_frame = _frame_maps(bmap, nplanes, h, w, dec, planes_per_frame)
    if out is None:
        out = torch.empty((nplanes, h, w), dtype=torch.int32, device=px.device)
    _need(out, torch.int32, "out")
    rows, cols = bmap.shape[1:]
    _check(lib().odhip_forward_partition(_p(out), _p(px), w, h * w, nplanes, w, h, int(dec), _p(bmap),
                                         cols, rows * cols, planes_per_frame, int(pic_w), int(pic_h),
                                         _stream()), "odhip_forward_partition")
    return out


def _frame_maps(bmap, nplanes, h, w, dec, planes_per_frame):
    """(bmap as [frames, rows, cols], planes_per_frame) of a CUDA map argument: one [rows, cols] map serves
    every plane."""
    import torch
    _need(bmap, torch.uint8, "bmap")
    planes_per_frame = int(planes_per_frame)
    if bmap.dim() == 2:
        bmap = bmap[None]
        planes_per_frame = nplanes
    if planes_per_frame < 1 or nplanes % planes_per_frame or tuple(bmap.shape) != (
            nplanes // planes_per_frame, (h << dec) // 8, (w << dec) // 8):
        raise DaalaHipError("bmap must be [%d / planes_per_frame, %d, %d]" % (nplanes, (h << dec) // 8, (w << dec) // 8))
    return bmap, planes_per_frame


def inverse_partition(coef, bmap, dec, pic_w, pic_h, planes_per_frame=1, out=None):
    """The decoder's reconstruction at each frame's own block-size map (odhip_inverse_partition): coef int32
    [nplanes, h, w] CUDA, dequantised, every leaf where it lies; bmap as for forward_partition.  Returns the
    pixels [nplanes, h, w] (uint8, int16 in a full-precision-references context)."""
    import torch
    _need(coef, torch.int32, "coef")
    nplanes, h, w = coef.shape
    bmap, planes_per_frame = _frame_maps(bmap, nplanes, h, w, dec, planes_per_frame)
    if out is None:
        out = torch.empty((nplanes, h, w), dtype=px_dtype(), device=coef.device)
    _need(out, px_dtype(), "out")
    rows, cols = bmap.shape[1:]
    _check(lib().odhip_inverse_partition(_p(out), w, h * w, _p(coef), nplanes, w, h, int(dec), _p(bmap), cols,
                                         rows * cols, planes_per_frame, int(pic_w), int(pic_h), _stream()),
           "odhip_inverse_partition")
    return out


def forward_partition_host(px, bmap, dec, pic_w, pic_h):
    """odhip_forward_partition_host: one plane on numpy arrays (uint8 [h, w] pixels, uint8 [rows, cols] map),
    synchronous.  Returns int32 [h, w]."""
    px = np.ascontiguousarray(px, dtype=np.uint8)
    bmap = np.ascontiguousarray(bmap, dtype=np.uint8)
    h, w = px.shape
    out = np.zeros((h, w), np.int32)
    _check(lib().odhip_forward_partition_host(out.ctypes.data_as(ctypes.c_void_p), px.ctypes.data_as(ctypes.c_void_p),
                                              w, w, h, int(dec), bmap.ctypes.data_as(ctypes.c_void_p), bmap.shape[1],
                                              int(pic_w), int(pic_h)), "odhip_forward_partition_host")
    return out


# ---- PVQ ---------------------------------------------------------------------
def pvq_search_batch(x, k, g2, pvq_norm_lambda, prev_k=None, y=None, cos=None):
    """Batched pvq_search_rdo_double.  x int16 [nbands, n], k int32 [nbands],
    g2 float64 [nbands]; returns (y int32 [nbands, n], cos float64 [nbands])."""
    import torch
    _need(x, torch.int16, "x")
    _need(k, torch.int32, "k")
    _need(g2, torch.float64, "g2")
    nbands, n = x.shape
    if y is None:
        y = torch.zeros((nbands, n), dtype=torch.int32, device=x.device)
    if cos is None:
        cos = torch.empty(nbands, dtype=torch.float64, device=x.device)
    pk = ctypes.c_void_p(None)
    if prev_k is not None:
        _need(prev_k, torch.int32, "prev_k")
        pk = _p(prev_k)
    _check(lib().odhip_pvq_search_batch(_p(x), int(n), _p(k), _p(y), _p(g2), pvq_norm_lambda, pk, _p(cos), nbands,
                                        _stream()), "odhip_pvq_search_batch")
    return y, cos


def copy_ceiling(nbytes=1 << 30, n=10):
    """odhip_copy_ceiling: the best of the library's three 16-byte-vector copy kernels, GB/s read + written."""
    best = 0.0
    for variant in range(3):
        g = ctypes.c_double()
        _check(lib().odhip_copy_ceiling(nbytes, int(n), variant, ctypes.byref(g), _stream()), "odhip_copy_ceiling")
        best = max(best, g.value)
    return best


def pvq_search_row_batch(x, k, g2, pvq_norm_lambda, force_scan=False):
    """odhip_pvq_search_row_batch: pvq_search_rdo_double one band per quad / 16-lane row (n = 31, 32,
    127, 128).  Returns (y int32 [nbands, n], cos float64 [nbands], replays int32 [nbands])."""
    import torch
    _need(x, torch.int16, "x")
    _need(k, torch.int32, "k")
    _need(g2, torch.float64, "g2")
    nbands, n = x.shape
    y = torch.zeros((nbands, n), dtype=torch.int32, device=x.device)
    cos = torch.empty(nbands, dtype=torch.float64, device=x.device)
    rep = torch.zeros(nbands, dtype=torch.int32, device=x.device)
    _check(lib().odhip_pvq_search_row_batch(_p(x), int(n), _p(k), _p(y), _p(g2), pvq_norm_lambda, int(bool(force_scan)),
                                            _p(cos), _p(rep), nbands, _stream()), "odhip_pvq_search_row_batch")
    return y, cos, rep


# ---- per-call host-pointer surfaces (numpy) ---------------------------------
class _Host:
    """The reference-signature entry points, callable on numpy arrays."""

    def dct2d(self, ln, x, inverse=False):
        n = 4 << ln
        x = np.ascontiguousarray(x, dtype=np.int32)
        assert x.shape == (n, n)
        out = np.zeros_like(x)
        name = "od_bin_%sdct%dx%d_hip" % ("i" if inverse else "f", n, n)
        getattr(lib(), name)(out.ctypes.data_as(ctypes.c_void_p), n,
                             x.ctypes.data_as(ctypes.c_void_p), n)
        return out

    def pvq_search(self, x, k, g2, lam, prev_k=0, y=None):
        x = np.ascontiguousarray(x, dtype=np.int16)
        n = x.shape[0]
        y = np.zeros(n, np.int32) if y is None else np.ascontiguousarray(y, np.int32)
        c = lib().od_pvq_search_rdo_double_hip(
            x.ctypes.data_as(ctypes.c_void_p), n, int(k),
            y.ctypes.data_as(ctypes.c_void_p), g2, lam, int(prev_k))
        return y, c


host = _Host()


# ---- PVQ band stage -----------------------------------------------------------
_CAND_FIELDS = ("band", "y", "choice", "cos_dist")

BAND_RECORD = np.dtype(_S["odhip_pvq_band"])        # one 64-byte record per (block, band)
assert BAND_RECORD.itemsize == 64
_Cands, _Job = _S["odhip_pvq_cands"], _S["odhip_pvq_job"]


def _addr(array):
    """The address of a host ctypes array, or None: for a pointer field, which does not keep the array alive."""
    return ctypes.addressof(array) if array is not None else None


# ---- with-reference (theta / Householder) building blocks -------------------------
REFPREP_RECORD, REFCAND_RECORD = np.dtype(_S["odhip_pvq_refprep"]), np.dtype(_S["odhip_pvq_refcand"])
MAX_REFCANDS, = _defines("PVQ_MAX_REFCANDS")
assert REFPREP_RECORD.itemsize == 64 and REFCAND_RECORD.itemsize == 24


def pvq_ref_prepare(x0, r0, qm, q0, beta, cfl_enabled):
    """x0, r0: int32 [nbands, n] CUDA; qm int16 [n].  Returns (x16, r16, xr, prep)
    with prep a uint8 [nbands, 64] tensor of odhip_pvq_refprep records."""
    import torch
    _need(x0, torch.int32, "x0")
    _need(r0, torch.int32, "r0")
    _need(qm, torch.int16, "qm")
    nbands, n = x0.shape
    dev = x0.device
    x16 = torch.empty((nbands, n), dtype=torch.int16, device=dev)
    r16 = torch.empty((nbands, n), dtype=torch.int16, device=dev)
    xr = torch.empty((nbands, n - 1), dtype=torch.int16, device=dev)
    prep = torch.empty((nbands, 64), dtype=torch.uint8, device=dev)
    _check(lib().odhip_pvq_ref_prepare(_p(x0), _p(r0), int(n), nbands, _p(qm),
                                       int(q0), int(beta), int(bool(cfl_enabled)), _p(x16), _p(r16),
                                       _p(xr), _p(prep), _stream()), "odhip_pvq_ref_prepare")
    return x16, r16, xr, prep


def pvq_ref_candidates(prep, theta, n, beta):
    """theta: int32 [nbands] = floor(.5 + OD_THETA_SCALE*acos(corr)) from the host.
    Returns (items uint8 [nbands, 24, 24] of odhip_pvq_refcand, nitems int32 [nbands])."""
    import torch
    _need(theta, torch.int32, "theta")
    nbands = prep.shape[0]
    items = torch.zeros((nbands, MAX_REFCANDS, 24), dtype=torch.uint8, device=prep.device)
    nitems = torch.empty(nbands, dtype=torch.int32, device=prep.device)
    _check(lib().odhip_pvq_ref_candidates(_p(prep), _p(theta), int(n), nbands, int(beta), _p(items), _p(nitems),
                                          _stream()), "odhip_pvq_ref_candidates")
    return items, nitems


def pvq_synthesis(y, r16, params, qm_inv):
    """od_pvq_synthesis_partial per band.  y int32 [nbands, n], r16 int16 [nbands, n],
    params int32 [nbands, 5] = (noref, g, theta, m, s), qm_inv int16 [n]."""
    import torch
    _need(y, torch.int32, "y")
    _need(r16, torch.int16, "r16")
    _need(params, torch.int32, "params")
    _need(qm_inv, torch.int16, "qm_inv")
    nbands, n = y.shape
    out = torch.empty_like(y)
    _check(lib().odhip_pvq_synthesis(_p(out), _p(y), _p(r16), int(n), nbands,
                                     _p(params), _p(qm_inv), _stream()), "odhip_pvq_synthesis")
    return out


def pvq_profile(enable):
    """Bracket the band stage's dominant kernel with HIP events (see daala_hip.h)."""
    _check(lib().odhip_pvq_profile(int(bool(enable))), "odhip_pvq_profile")


def pvq_profile_read(max_n=256):
    """Milliseconds of every bracketed launch since the last read."""
    buf = (ctypes.c_float * max_n)()
    n = lib().odhip_pvq_profile_read(buf, max_n)
    if n < 0:
        raise DaalaHipError("odhip_pvq_profile_read failed with code %d" % n)
    return [buf[i] for i in range(n)]


def pvq_band_layout(bs):
    """(nb_bands, offsets[nb_bands + 1], len) for block size 4 << bs."""
    nb = ctypes.c_int()
    offs = (ctypes.c_int * 13)()
    ln = ctypes.c_int()
    _check(lib().odhip_pvq_band_layout(int(bs), ctypes.byref(nb), offs, ctypes.byref(ln)),
           "odhip_pvq_band_layout")
    return nb.value, [offs[i] for i in range(nb.value + 1)], ln.value


def alloc_pvq_cands(nblocks, bs, device, cos_dist=False):
    """Device buffers of odhip_pvq_cands: 'band' is the [B][nb] array of 64-byte
    odhip_pvq_band records (as bytes; unpack_cands decodes it), 'y' the int16
    pulse vectors [2][B][len], 'choice' [B][nb][4]; 'cos_dist' [B][nb][2] only on
    request (parity checks)."""
    import torch
    nb, _, ln = pvq_band_layout(bs)
    out = {
        "band": torch.zeros((nblocks, nb, 64), dtype=torch.uint8, device=device),
        "y": torch.zeros((2, nblocks, ln), dtype=torch.int16, device=device),
        "choice": torch.empty((nblocks, nb, 4), dtype=torch.int32, device=device),
        "cos_dist": None,
    }
    if cos_dist:
        out["cos_dist"] = torch.zeros((nblocks, nb, 2), dtype=torch.float64, device=device)
    return out


def unpack_cands(cands):
    """Host copy of a cands dict as numpy arrays keyed by field name: the record
    fields (cg, gain, k, flags, dist0, yy, dist, moment: [B][nb] or [B][nb][2]) plus y,
    choice and, when present, cos_dist."""
    rec = cands["band"].cpu().numpy().view(BAND_RECORD)[..., 0]
    out = {name: np.ascontiguousarray(rec[name]) for name in
           ("cg", "gain", "k", "flags", "dist0", "yy", "dist", "moment")}
    out["y"] = cands["y"].cpu().numpy()
    out["choice"] = cands["choice"].cpu().numpy()
    if cands.get("cos_dist") is not None:
        out["cos_dist"] = cands["cos_dist"].cpu().numpy()
    return out


class PvqJob:
    """One (plane set, block size) unit of the PVQ band stage.  It owns every tensor and host array (q_band,
    beta_band, q_band2) that its struct() points to: the struct keeps none of them alive, so the job has to outlive
    every call that is handed its struct."""

    def __init__(self, coef, bs, qm, qm_inv, q_band, beta_band, cands=None, dq=None,
                 rate=None, qg=None, q_band2=None, plane_split=0):
        """q_band2 / plane_split: the planes from plane_split on (the Cr half of a chroma
        plane set) take q_band2 - pvq_qm_q4[pli] is per plane in the reference."""
        import torch
        _need(coef, torch.int32, "coef")
        self.coef, self.bs, self.qm, self.qm_inv = coef, int(bs), qm, qm_inv
        nplanes, h, w = coef.shape
        n = 4 << bs
        self.nblocks = nplanes * (h // n) * (w // n)
        nb = pvq_band_layout(bs)[0]
        assert len(q_band) == nb and len(beta_band) == nb
        self.q_band = (ctypes.c_int32 * 12)(*[int(v) for v in q_band])
        self.beta_band = (ctypes.c_int32 * 12)(*[int(v) for v in beta_band])
        self.q_band2 = (ctypes.c_int32 * 12)(*[int(v) for v in q_band2]) if q_band2 is not None else None
        self.plane_split = int(plane_split) if q_band2 is not None else 0
        self.cands = cands if cands is not None else alloc_pvq_cands(self.nblocks, bs,
                                                                     coef.device)
        self.dq, self.rate, self.qg = dq, rate, qg
        for t, dt, what in ((qm, torch.int16, "qm"), (qm_inv, torch.int16, "qm_inv"),
                            (dq, torch.int32, "dq"), (rate, torch.float64, "rate"),
                            (qg, torch.int32, "qg")):
            if t is not None:
                _need(t, dt, what)

    def struct(self):
        opt = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)  # noqa: E731
        nplanes, h, w = self.coef.shape
        c = _Cands(*[ctypes.c_void_p(self.cands[n].data_ptr() if self.cands.get(n) is not None
                                     else None) for n in _CAND_FIELDS])
        return _Job(d_coef=_p(self.coef), nplanes=nplanes, w=w, h=h, bs=self.bs, d_qm=opt(self.qm),
                    d_qm_inv=opt(self.qm_inv), q_band=_addr(self.q_band), beta_band=_addr(self.beta_band), cands=c,
                    d_dq=opt(self.dq), d_rate=opt(self.rate), d_qg=opt(self.qg), q_band2=_addr(self.q_band2),
                    plane_split=self.plane_split)


def _jobs_array(jobs):
    arr = (_Job * len(jobs))()
    for i, j in enumerate(jobs):
        arr[i] = j.struct()
    return arr


def pvq_noref_bands_multi(jobs, pvq_norm_lambda):
    """The adaptation-independent part of pvq_theta (no-reference path) for every
    block and band of every job, in one set of launches."""
    _check(lib().odhip_pvq_noref_bands_multi(_jobs_array(jobs), len(jobs), pvq_norm_lambda, _stream()),
           "odhip_pvq_noref_bands_multi")


def pvq_select_synth_noref_multi(jobs, pvq_norm_lambda):
    """Choice (`cost <= best_cost`, cost = dist + lambda*rate) + decoder-identical
    dequantisation into each job's dq plane."""
    _check(lib().odhip_pvq_select_synth_noref_multi(_jobs_array(jobs), len(jobs), pvq_norm_lambda, _stream()),
           "odhip_pvq_select_synth_noref_multi")


def pvq_choose_multi(jobs, pvq_norm_lambda):
    """The `cost <= best_cost` choice alone (fills cands['choice'])."""
    _check(lib().odhip_pvq_choose_multi(_jobs_array(jobs), len(jobs), pvq_norm_lambda, _stream()),
           "odhip_pvq_choose_multi")


def _resolved(n, what):
    if n < 0:
        raise DaalaHipError("%s failed with code %d" % (what, n))
    return n


def pvq_choose_priced_multi(jobs, pvq_norm_lambda, fused_bands=False):
    """The choice priced with od_pvq_rate's closed form on the device.  fused_bands=False:
    after pvq_noref_bands_multi, a choice kernel reads the records
    (odhip_pvq_choose_priced_multi); True: band stage AND choice in one pass
    (odhip_pvq_noref_bands_priced_multi).  Either way followed by the host-libm resolve;
    returns the number of bands it re-decided."""
    arr = _jobs_array(jobs)
    if fused_bands:
        _check(lib().odhip_pvq_noref_bands_priced_multi(arr, len(jobs), pvq_norm_lambda, _stream()),
               "odhip_pvq_noref_bands_priced_multi")
    else:
        _check(lib().odhip_pvq_choose_priced_multi(arr, len(jobs), pvq_norm_lambda, _stream()),
               "odhip_pvq_choose_priced_multi")
    return _resolved(lib().odhip_pvq_choose_priced_resolve(arr, len(jobs), pvq_norm_lambda, _stream()),
                     "odhip_pvq_choose_priced_resolve")


def inverse_level_pvq(job, dec, pic_w, pic_h, out=None):
    """Inverse stage fed by the band stage: dequantise-on-load from the chosen
    pulse vectors of `job` (no dequantised plane in HBM)."""
    import torch
    nplanes, h, w = job.coef.shape
    if out is None:
        out = torch.empty((nplanes, h, w), dtype=px_dtype(), device=job.coef.device)
    st = job.struct()
    _check(lib().odhip_inverse_level_pvq(_p(out), w, h * w, ctypes.byref(st), int(dec), int(pic_w), int(pic_h),
                                         _stream()), "odhip_inverse_level_pvq")
    return out


def inverse_levels_pvq(jobs, dec, pic_w, pic_h, outs=None):
    """inverse_level_pvq for several levels of one plane set in one set of launches;
    returns the list of reconstructed uint8 [nplanes, h, w] tensors."""
    import torch
    nplanes, h, w = jobs[0].coef.shape
    if outs is None:
        outs = [torch.empty((nplanes, h, w), dtype=px_dtype(), device=jobs[0].coef.device)
                for _ in jobs]
    ptrs = (ctypes.c_void_p * len(jobs))(*[o.data_ptr() for o in outs])
    _check(lib().odhip_inverse_levels_pvq(ptrs, w, h * w, _jobs_array(jobs), len(jobs), int(dec), int(pic_w),
                                          int(pic_h), _stream()), "odhip_inverse_levels_pvq")
    return outs


def pvq_noref_bands(coef, bs, qm, q_band, beta_band, pvq_norm_lambda, out=None, cos_dist=False):
    if out is None and cos_dist:
        nplanes, h, w = coef.shape
        n = 4 << bs
        out = alloc_pvq_cands(nplanes * (h // n) * (w // n), bs, coef.device, cos_dist=True)
    job = PvqJob(coef, bs, qm, None, q_band, beta_band, cands=out)
    pvq_noref_bands_multi([job], pvq_norm_lambda)
    return job.cands


def pvq_select_synth_noref(coef, bs, qm_inv, q_band, beta_band, pvq_norm_lambda, cands,
                           rate=None, dq=None, qg=None):
    import torch
    if dq is None:
        dq = torch.empty_like(coef)
    if qg is None:
        qg = torch.empty(tuple(cands["band"].shape[:2]), dtype=torch.int32, device=coef.device)
    job = PvqJob(coef, bs, None, qm_inv, q_band, beta_band, cands=cands, dq=dq, rate=rate, qg=qg)
    pvq_select_synth_noref_multi([job], pvq_norm_lambda)
    return dq, qg


# ---- with-reference band stage on whole planes (odhip_pvq_ref_bands_multi) ---------
REF_SLOTS, = _defines("PVQ_REF_SLOTS")
REFBAND_RECORD, REFITEM_RECORD = np.dtype(_S["odhip_pvq_refband"]), np.dtype(_S["odhip_pvq_refitem"])
assert REFBAND_RECORD.itemsize == 64 and REFITEM_RECORD.itemsize == 48
REFBAND_R_NULL, REFBAND_THETA, REFBAND_NOREF, REFBAND_FLIP, REFBAND_UNCERTAIN = _defines(
    "REFBAND_R_NULL", "REFBAND_THETA", "REFBAND_NOREF", "REFBAND_FLIP", "REFBAND_UNCERTAIN")
REFITEM_SEARCHED, REFITEM_WITH_REF, REFITEM_K_RANGE, REFITEM_MOMENT_SHIFT = _defines(
    "REFITEM_SEARCHED", "REFITEM_WITH_REF", "REFITEM_K_RANGE", "REFITEM_MOMENT_SHIFT")
_RefJob = _S["odhip_pvq_refjob"]


class PvqRefJob:
    """One (plane set, reference plane set, block size) unit of the with-reference band stage (odhip_pvq_refjob).
    It owns its output and work buffers and the host arrays q_band, beta_band and q_band2 that its struct() points
    to: the struct keeps none of them alive, so the job has to outlive every call that is handed its struct."""

    def __init__(self, coef, ref, bs, qm, qm_inv, q_band, beta_band, is_keyframe, pli, rate=None,
                 share=None, q_band2=None, plane_split=0):
        """share: another PvqRefJob of the same shape whose output and work buffers this
        one uses too (same planes, another reference buffer: double-buffered references)."""
        import torch
        _need(coef, torch.int32, "coef")
        _need(ref, torch.int32, "ref")
        assert coef.shape == ref.shape
        self.coef, self.ref, self.bs, self.qm, self.qm_inv = coef, ref, int(bs), qm, qm_inv
        self.is_keyframe, self.pli, self.rate = int(is_keyframe), int(pli), rate
        nplanes, h, w = coef.shape
        n = 4 << bs
        self.nblocks = B = nplanes * (h // n) * (w // n)
        self.nb, self.offsets, self.len = pvq_band_layout(bs)
        assert len(q_band) == self.nb and len(beta_band) == self.nb
        self.q_band = (ctypes.c_int32 * 12)(*[int(v) for v in q_band])
        self.beta_band = (ctypes.c_int32 * 12)(*[int(v) for v in beta_band])
        self.q_band2 = (ctypes.c_int32 * 12)(*[int(v) for v in q_band2]) if q_band2 is not None else None
        self.plane_split = int(plane_split) if q_band2 is not None else 0
        dev = coef.device
        if share is not None:
            assert share.coef.shape == coef.shape and share.bs == self.bs
            for f in ("band", "items", "y", "r16", "x16", "xr", "choice", "dq"):
                setattr(self, f, getattr(share, f))
            return
        self.band = torch.zeros((B, self.nb, 64), dtype=torch.uint8, device=dev)
        self.items = torch.zeros((3, self.nb, REF_SLOTS, B, 16), dtype=torch.uint8, device=dev)
        self.y = torch.zeros((REF_SLOTS, B, self.len), dtype=torch.int16, device=dev)
        self.r16 = torch.zeros((B, self.len), dtype=torch.int16, device=dev)
        self.x16 = torch.zeros((B, self.len), dtype=torch.int16, device=dev)
        self.xr = torch.zeros((B, self.len), dtype=torch.int16, device=dev)
        self.choice = torch.zeros((B, self.nb, 16), dtype=torch.int32, device=dev)
        self.dq = torch.zeros_like(coef)
        for t, dt, what in ((qm, torch.int16, "qm"), (qm_inv, torch.int16, "qm_inv"),
                            (rate, torch.float64, "rate")):
            if t is not None:
                _need(t, dt, what)

    def struct(self):
        opt = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)  # noqa: E731
        nplanes, h, w = self.coef.shape
        return _RefJob(d_coef=_p(self.coef), d_ref=_p(self.ref), nplanes=nplanes, w=w, h=h, bs=self.bs,
                       is_keyframe=self.is_keyframe, pli=self.pli, d_qm=opt(self.qm), d_qm_inv=opt(self.qm_inv),
                       q_band=_addr(self.q_band), beta_band=_addr(self.beta_band), band=_p(self.band),
                       items=_p(self.items), y=_p(self.y), r16=_p(self.r16), x16=_p(self.x16), xr=_p(self.xr),
                       d_rate=opt(self.rate), choice=_p(self.choice), d_dq=_p(self.dq),
                       q_band2=_addr(self.q_band2), plane_split=self.plane_split)

    def unpack(self):
        """Host copies: record fields [B][nb], item fields [B][nb][REF_SLOTS], y, choice."""
        rec = self.band.cpu().numpy().view(REFBAND_RECORD)[..., 0]
        # three planes of 16-byte vectors [part][nb][slot][B] -> records [B][nb][slot]
        raw = self.items.cpu().numpy()
        items = np.zeros(raw.shape[1:4], REFITEM_RECORD)
        head = raw[0].view("<i4")
        tail = raw[1].view("<i4")
        res = raw[2].view("<f8")
        for i, f in enumerate(("gain", "theta", "ts", "k")):
            items[f] = head[..., i]
        for i, f in enumerate(("qcg", "qtheta", "flags", "yslot")):
            items[f] = tail[..., i]
        items["cos_dist"] = res[..., 0]
        items["dist"] = res[..., 1]
        items = np.ascontiguousarray(items.transpose(2, 0, 1))
        return {"rec": rec, "items": items, "y": self.y.cpu().numpy(),
                "choice": self.choice.cpu().numpy(), "r16": self.r16.cpu().numpy(),
                "x16": self.x16.cpu().numpy(), "xr": self.xr.cpu().numpy()}


def _refjobs_array(jobs):
    arr = (_RefJob * len(jobs))()
    for i, j in enumerate(jobs):
        arr[i] = j.struct()
    return arr


def pvq_ref_bands_multi(jobs, pvq_norm_lambda, resolve=True):
    """pvq_theta with a reference up to the rate-dependent choice, for every block
    and band of every job; resolve=True also settles the bands whose theta is
    inside the device-acos margin with the host libm (returns how many were
    re-run)."""
    arr = _refjobs_array(jobs)
    _check(lib().odhip_pvq_ref_bands_multi(arr, len(jobs), pvq_norm_lambda, _stream()), "odhip_pvq_ref_bands_multi")
    if not resolve:
        return 0
    if resolve == "async":
        _check(lib().odhip_pvq_ref_resolve_begin(_stream()), "odhip_pvq_ref_resolve_begin")
        return 0
    n = lib().odhip_pvq_ref_resolve(arr, len(jobs), pvq_norm_lambda, _stream())
    if n < 0:
        raise DaalaHipError("odhip_pvq_ref_resolve failed with code %d" % n)
    return n


def pvq_ref_resolve_finish(jobs, pvq_norm_lambda):
    """Second half of pvq_ref_bands_multi(..., resolve="async"): waits for the count
    of bands inside the device-acos margin only; 0 (normal) or the number of bands
    re-run with the host's theta - then the caller repeats choice / synthesis."""
    n = lib().odhip_pvq_ref_resolve_finish(_refjobs_array(jobs), len(jobs), pvq_norm_lambda, _stream())
    if n < 0:
        raise DaalaHipError("odhip_pvq_ref_resolve_finish failed with code %d" % n)
    return n


def pvq_ref_select_synth_multi(jobs, pvq_norm_lambda):
    """The reference's choice among the candidates (cost = dist + lambda*rate, rate
    table optional), skip rules and decoder-identical synthesis into job.dq."""
    _check(lib().odhip_pvq_ref_select_synth_multi(_refjobs_array(jobs), len(jobs), pvq_norm_lambda, _stream()),
           "odhip_pvq_ref_select_synth_multi")


# ---- the band stages on the leaves of a block-size map (odhip_partition_*) -----------------
NBSIZES, = _defines("NBSIZES")


class PartitionLeaves:
    """The leaf lists of a plane set [nplanes, h, w] at its block-size maps (include/daala_hip.h, "the PVQ band
    stages on the leaves of a block-size map").  lists: every list in one array - int32 CUDA
    (partition_leaves) or numpy uint32 (partition_leaves_host); counts: numpy int32 [5, nplanes]."""

    def __init__(self, lists, counts, nplanes, h, w, dec):
        self.lists, self.counts = lists, counts
        self.nplanes, self.h, self.w, self.dec = nplanes, h, w, int(dec)

    @staticmethod
    def entries(nplanes, h, w, dec):
        return sum(nplanes * (w // (4 << s)) * (h // (4 << s)) for s in range(NBSIZES - dec))

    def cap(self, s):
        return (self.w // (4 << s)) * (self.h // (4 << s))

    def list(self, s):
        """[nplanes, cap(s)]: row p holds the ascending block indices of plane p's leaves of size s in its
        first counts[s, p] entries."""
        off = sum(self.nplanes * self.cap(t) for t in range(s))
        return self.lists[off:off + self.nplanes * self.cap(s)].reshape(self.nplanes, self.cap(s))

    def sizes(self):
        """The sizes that have a leaf (a dense set, a job)."""
        return [s for s in range(NBSIZES - self.dec) if self.counts[s].any()]

    def dense_rows(self, s):
        """Hd_s: the rows of a dense plane of size s."""
        nbx = self.w // (4 << s)
        return (4 << s) * int(-(-int(self.counts[s].max()) // nbx))


def _np_p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def partition_leaves_host(bmap, nplanes, h, w, dec, planes_per_frame=1):
    """odhip_partition_leaves_host: the leaf lists of nplanes planes of h x w from numpy maps - uint8
    [frames, rows, cols], or one [rows, cols] map for every plane; a view with wider rows or frames is passed
    with its own strides.  No GPU is touched."""
    bmap = np.asarray(bmap)
    if bmap.ndim == 2:
        bmap = bmap[None]
        planes_per_frame = nplanes
    if bmap.dtype != np.uint8 or bmap.ndim != 3 or bmap.strides[2] != 1:
        raise DaalaHipError("bmap must be uint8 [frames, rows, cols] with contiguous rows")
    lists = np.zeros(max(PartitionLeaves.entries(nplanes, h, w, dec), 1), np.uint32)
    counts = np.zeros((NBSIZES, nplanes), np.int32)
    _check(lib().odhip_partition_leaves_host(_np_p(lists), _np_p(counts), nplanes, w, h, int(dec), _np_p(bmap),
                                             bmap.strides[1], bmap.strides[0], int(planes_per_frame)),
           "odhip_partition_leaves_host")
    return PartitionLeaves(lists, counts, nplanes, h, w, dec)


def partition_leaves(bmap, nplanes, h, w, dec, planes_per_frame=1):
    """odhip_partition_leaves: the same from CUDA maps (as for forward_partition) into CUDA lists.  The counts
    come back to the host: the call waits for the current stream."""
    import torch
    bmap, planes_per_frame = _frame_maps(bmap, nplanes, h, w, dec, planes_per_frame)
    lists = torch.zeros(max(PartitionLeaves.entries(nplanes, h, w, dec), 1), dtype=torch.int32, device=bmap.device)
    counts = np.zeros((NBSIZES, nplanes), np.int32)
    rows, cols = bmap.shape[1:]
    _check(lib().odhip_partition_leaves(_p(lists), _np_p(counts), nplanes, w, h, int(dec), _p(bmap), cols,
                                        rows * cols, planes_per_frame, _stream()), "odhip_partition_leaves")
    return PartitionLeaves(lists, counts, nplanes, h, w, dec)


def _partition_copy(fn, dst, src, s, leaves):
    counts = np.ascontiguousarray(leaves.counts[s])
    _check(fn(_p(dst), _p(src), int(s), _p(leaves.list(s)), _np_p(counts), leaves.nplanes, leaves.w, leaves.h,
              leaves.dec, _stream()), fn.__name__)


def partition_gather(src, leaves, s, out=None):
    """odhip_partition_gather: the leaves of size s of src (int32 [nplanes, h, w] CUDA: coefficients, or a
    reference at the same maps) as the dense set int32 [nplanes, Hd_s, w], zero padding included.  A size
    without a leaf gives an empty set and launches nothing."""
    import torch
    _need(src, torch.int32, "src")
    if tuple(src.shape) != (leaves.nplanes, leaves.h, leaves.w):
        raise DaalaHipError("src must be [%d, %d, %d]" % (leaves.nplanes, leaves.h, leaves.w))
    hd = leaves.dense_rows(s)
    if out is None:
        out = torch.empty((leaves.nplanes, hd, leaves.w), dtype=torch.int32, device=src.device)
    _need(out, torch.int32, "out")
    if tuple(out.shape) != (leaves.nplanes, hd, leaves.w):
        raise DaalaHipError("out must be [%d, %d, %d]" % (leaves.nplanes, hd, leaves.w))
    if hd:
        _partition_copy(lib().odhip_partition_gather, out, src, s, leaves)
    return out


def partition_scatter(dst, dense, leaves, s):
    """odhip_partition_scatter: the blocks of the dense set of size s back to their leaves in dst (int32
    [nplanes, h, w] CUDA); nothing else of dst is written."""
    import torch
    _need(dst, torch.int32, "dst")
    _need(dense, torch.int32, "dense")
    hd = leaves.dense_rows(s)
    if tuple(dst.shape) != (leaves.nplanes, leaves.h, leaves.w) or tuple(dense.shape) != (leaves.nplanes, hd, leaves.w):
        raise DaalaHipError("dst must be [%d, %d, %d], dense [.., %d, ..]" % (leaves.nplanes, leaves.h, leaves.w, hd))
    if hd:
        _partition_copy(lib().odhip_partition_scatter, dst, dense, s, leaves)
    return dst


class PartitionPvq:
    """What pvq_partition_noref / pvq_partition_ref return: dq, the dequantised planes int32 [nplanes, h, w] in
    the layout inverse_partition reads; leaves, the PartitionLeaves; jobs {s: PvqJob or PvqRefJob} over the
    dense set of every size present - their candidate, pulse and choice buffers index the dense blocks: block
    blk = (p*(Hd_s/N) + i // (w/N))*(w/N) + i % (w/N) is leaf leaves.list(s)[p, i]."""

    def __init__(self, dq, leaves, jobs):
        self.dq, self.leaves, self.jobs = dq, leaves, jobs


def pvq_partition_noref(coef, bmap, dec, tables, pvq_norm_lambda, planes_per_frame=1, plane_split=0, price=None):
    """The no-reference band stage on every leaf of coef (forward_partition's planes) at its own size: leaf
    lists, one gather per size, ONE odhip_pvq_noref_bands_multi + odhip_pvq_select_synth_noref_multi over the
    sizes present, scatter.  tables[s] = (qm, qm_inv, q_band, beta_band[, q_band2]) as for PvqJob
    (QuantTables.size_tables); q_band2 goes with plane_split.  price(jobs): optional, called between the two
    stages to set each job's rate table (the host entropy model); without it the choice is on distortion alone.
    Returns a PartitionPvq."""
    import torch
    _need(coef, torch.int32, "coef")
    leaves = partition_leaves(bmap, coef.shape[0], coef.shape[1], coef.shape[2], dec, planes_per_frame)
    sizes = leaves.sizes()
    jobs = {}
    for s in sizes:
        dense = partition_gather(coef, leaves, s)
        t = tables[s]
        jobs[s] = PvqJob(dense, s, t[0], t[1], t[2], t[3], dq=torch.empty_like(dense),
                         q_band2=t[4] if len(t) > 4 else None, plane_split=plane_split)
    dq = torch.zeros_like(coef)
    if jobs:
        order = [jobs[s] for s in sizes]
        pvq_noref_bands_multi(order, pvq_norm_lambda)
        if price is not None:
            price(jobs)
        pvq_select_synth_noref_multi(order, pvq_norm_lambda)
        for s in sizes:
            partition_scatter(dq, jobs[s].dq, leaves, s)
    return PartitionPvq(dq, leaves, jobs)


def pvq_partition_ref(coef, ref, bmap, dec, tables, pvq_norm_lambda, is_keyframe, pli, planes_per_frame=1,
                      plane_split=0, price=None):
    """The with-reference band stage on every leaf: as pvq_partition_noref through odhip_pvq_ref_bands_multi,
    odhip_pvq_ref_resolve and odhip_pvq_ref_select_synth_multi, with ref (forward_partition of the prediction at
    the same maps) gathered by the same lists.  Returns a PartitionPvq; reruns = the bands the resolve settled."""
    import torch
    _need(coef, torch.int32, "coef")
    _need(ref, torch.int32, "ref")
    if ref.shape != coef.shape:
        raise DaalaHipError("ref must have the shape of coef")
    leaves = partition_leaves(bmap, coef.shape[0], coef.shape[1], coef.shape[2], dec, planes_per_frame)
    sizes = leaves.sizes()
    jobs = {}
    for s in sizes:
        t = tables[s]
        jobs[s] = PvqRefJob(partition_gather(coef, leaves, s), partition_gather(ref, leaves, s), s, t[0], t[1], t[2],
                            t[3], is_keyframe, pli, q_band2=t[4] if len(t) > 4 else None, plane_split=plane_split)
    dq = torch.zeros_like(coef)
    out = PartitionPvq(dq, leaves, jobs)
    out.reruns = 0
    if jobs:
        order = [jobs[s] for s in sizes]
        out.reruns = pvq_ref_bands_multi(order, pvq_norm_lambda, resolve=True)
        if price is not None:
            price(jobs)
        pvq_ref_select_synth_multi(order, pvq_norm_lambda)
        for s in sizes:
            partition_scatter(dq, jobs[s].dq, leaves, s)
    return out


def cfl_refs_partition(luma, bmap, dec, planes_per_frame=2, out=None):
    """odhip_cfl_refs_partition: the chroma-from-luma reference planes of keyframe chroma at a block-size map.
    luma: int32 [nplanes, h, w] CUDA, DEQUANTISED (pvq_partition_noref(...).dq); bmap: uint8 [nplanes, h/8, w/8]
    CUDA, or one [h/8, w/8] map for every plane.  Returns int32 [nplanes*planes_per_frame, h >> dec, w >> dec]:
    plane q predicted from luma plane q // planes_per_frame - the `ref` of pvq_partition_ref on chroma planes
    laid out the same way.  At dec = 0 every plane is a copy of its luma plane; a 4:4:4 caller may pass the luma
    planes as the reference instead."""
    import torch
    _need(luma, torch.int32, "luma")
    nplanes, h, w = luma.shape
    dec, planes_per_frame = int(dec), int(planes_per_frame)
    one = bmap.dim() == 2                    # one map for every plane: a frame stride of zero
    bmap, _ = _frame_maps(bmap, nplanes, h, w, 0, 1)
    shape = (nplanes * max(planes_per_frame, 0), h >> (dec & 1), w >> (dec & 1))
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=luma.device)
    _need(out, torch.int32, "out")
    if tuple(out.shape) != shape:
        raise DaalaHipError("out must be [%d, %d, %d]" % shape)
    rows, cols = bmap.shape[1:]
    _check(lib().odhip_cfl_refs_partition(_p(out), _p(luma), nplanes, w, h, dec, _p(bmap), cols,
                                          0 if one else rows * cols, planes_per_frame, _stream()),
           "odhip_cfl_refs_partition")
    return out


def cfl_refs_partition_host(luma, bmap, dec):
    """odhip_cfl_refs_partition_host: one plane on numpy arrays, no GPU.  luma int32 [h, w] (dequantised), bmap
    uint8 [h/8, w/8] (a view with wider rows is passed with its stride).  Returns int32 [h >> dec, w >> dec]."""
    luma = np.ascontiguousarray(luma, dtype=np.int32)
    bmap = np.asarray(bmap)
    if luma.ndim != 2 or bmap.dtype != np.uint8 or bmap.ndim != 2 or bmap.strides[1] != 1:
        raise DaalaHipError("luma must be int32 [h, w], bmap uint8 [rows, cols] with contiguous rows")
    h, w = luma.shape
    if bmap.shape[0] < h // 8 or bmap.shape[1] < w // 8:
        raise DaalaHipError("bmap must hold %d x %d entries" % (h // 8, w // 8))
    dec = int(dec)
    ref = np.zeros((h >> (dec & 1), w >> (dec & 1)), np.int32)
    _check(lib().odhip_cfl_refs_partition_host(_np_p(ref), _np_p(luma), w, h, dec, _np_p(bmap), bmap.strides[0]),
           "odhip_cfl_refs_partition_host")
    return ref


def keyframe_partition_420(luma_px, cb_px, cr_px, bmap, quant_tables, pvq_norm_lambda, pic_w, pic_h, price=None):
    """A 4:2:0 keyframe coded at its block-size map from the library's own calls, chained and nothing else:
    forward_partition of the three plane sets, pvq_partition_noref on luma, cfl_refs_partition of its dq,
    pvq_partition_ref(is_keyframe=1, pli=1 / 2) on Cb and Cr against those planes, inverse_partition of the three
    dq.  luma_px [F, h, w], cb_px, cr_px [F, h/2, w/2]: padded pixel planes (px_dtype()) on CUDA; bmap uint8
    [F, h/8, w/8] CUDA (bsize_decide's map) or one [h/8, w/8] map; quant_tables: a QuantTables; pic_w, pic_h: the
    unpadded luma picture size.  price(pli, jobs): optional, called between the band stage and the choice of plane
    pli to set each job's rate table.
    Keyframe luma goes through the NO-REFERENCE stage, as the frame-batch pipe codes it (no HV intra prediction),
    and the DCs pass through the band stages unchanged (the keyframe Haar-DC tree is not built).
    Returns (pvq, ref, recon): pvq = [PartitionPvq of Y, Cb, Cr], ref = the reference planes int32 [F, h/2, w/2]
    that Cb and Cr share, recon = [pixels of Y, Cb, Cr]."""
    px = (luma_px, cb_px, cr_px)
    hook = (lambda pli: None) if price is None else (lambda pli: lambda jobs: price(pli, jobs))
    coef = [forward_partition(px[pli], bmap, int(pli > 0), pic_w, pic_h) for pli in range(3)]
    pvq = [pvq_partition_noref(coef[0], bmap, 0, quant_tables.size_tables(0, 0), pvq_norm_lambda, price=hook(0))]
    ref = cfl_refs_partition(pvq[0].dq, bmap, 1, planes_per_frame=1)
    for pli in (1, 2):
        pvq.append(pvq_partition_ref(coef[pli], ref, bmap, 1, quant_tables.size_tables(pli, 1), pvq_norm_lambda, 1, pli,
                                     price=hook(pli)))
    recon = [inverse_partition(pvq[pli].dq, bmap, int(pli > 0), pic_w, pic_h) for pli in range(3)]
    return pvq, ref, recon


# Test hooks live in the library's contexts (odhip_ctx_set_test_hooks); this module keeps the
# values the tests asked for and applies them to the calling thread's current context and to
# every live Pipe (and to Pipes made later).
_hooks = {"margin": 0.0, "perturb": 0, "tol": 1.0}
_pipes = None


def _apply_hooks():
    global _pipes
    import weakref
    if _pipes is None:
        _pipes = weakref.WeakSet()
    L = lib()
    args = (_hooks["margin"], int(_hooks["perturb"]), _hooks["tol"])
    _check(L.odhip_ctx_set_test_hooks(None, *args), "odhip_ctx_set_test_hooks")
    for p in list(_pipes):
        if p.h:
            _check(L.odhip_pipe_set_test_hooks(p._p(), *args), "odhip_pipe_set_test_hooks")


def pvq_ref_set_theta_margin(margin, perturb=False):
    """Test hook (per context in the library): the device-acos uncertainty margin (<= 0: the
    default) and a deliberately wrong device theta for the listed bands."""
    _hooks["margin"] = float(margin)
    _hooks["perturb"] = int(bool(perturb))
    _apply_hooks()


def pvq_ref_theta_probe(corr):
    """.5 + OD_THETA_SCALE*acos(corr) as the device evaluates it."""
    import torch
    _need(corr, torch.float64, "corr")
    out = torch.empty_like(corr)
    _check(lib().odhip_pvq_ref_theta_probe(_p(corr), _p(out), corr.numel(), _stream()), "odhip_pvq_ref_theta_probe")
    return out


def pvq_ref_profile(enable):
    _check(lib().odhip_pvq_ref_profile(int(bool(enable))), "odhip_pvq_ref_profile")


def pvq_ref_profile_read(max_n=256):
    """Milliseconds of each k_refb_search_row<8> launch recorded since the last read."""
    buf = (ctypes.c_float * max_n)()
    n = lib().odhip_pvq_ref_profile_read(buf, max_n)
    if n < 0:
        raise DaalaHipError("odhip_pvq_ref_profile_read failed with code %d" % n)
    return [buf[i] for i in range(n)]


def image_planes_copy_pad(src, plane_w, plane_h, out=None):
    """od_img_plane_copy_pad for a batch of planes: src uint8 [nplanes, pic_h, pic_w]
    -> uint8 [nplanes, plane_h, plane_w] (picture copied, padding low-pass
    extended as the reference's input queue does)."""
    import torch
    _need(src, torch.uint8, "src")
    nplanes, pic_h, pic_w = src.shape
    if out is None:
        out = torch.empty((nplanes, plane_h, plane_w), dtype=torch.uint8, device=src.device)
    _check(lib().odhip_image_planes_copy_pad(_p(out), plane_w, plane_h * plane_w, plane_w, plane_h,
                                             _p(src) if src.numel() else None, pic_w, pic_h * pic_w, pic_w, pic_h,
                                             nplanes, _stream()), "odhip_image_planes_copy_pad")
    return out


def image_planes_copy_pad16(src, plane_w, plane_h, src_bitdepth=8, out=None):
    """od_img_plane_copy_pad for an encoder with full-precision references: src uint8
    (src_bitdepth 8) or int16 (10 / 12) [nplanes, pic_h, pic_w] -> int16 samples at 12 bits
    [nplanes, plane_h, plane_w]."""
    import torch
    _need(src, torch.uint8 if src_bitdepth == 8 else torch.int16, "src")
    nplanes, pic_h, pic_w = src.shape
    if out is None:
        out = torch.empty((nplanes, plane_h, plane_w), dtype=torch.int16, device=src.device)
    _check(lib().odhip_image_planes_copy_pad16(_p(out), plane_w, plane_h * plane_w, plane_w, plane_h,
                                               _p(src) if src.numel() else None, int(src_bitdepth), pic_w,
                                               pic_h * pic_w, pic_w, pic_h, nplanes, _stream()),
           "odhip_image_planes_copy_pad16")
    return out


def inverse_levels(coefs, dec, leaf_bs, pic_w, pic_h, outs=None):
    """inverse_level for several partition levels of one plane set in one set of
    launches: coefs[i] (int32 [nplanes, h, w]) at level leaf_bs[i] -> outs[i]."""
    import torch
    nplanes, h, w = coefs[0].shape
    if outs is None:
        outs = [torch.empty((nplanes, h, w), dtype=px_dtype(), device=coefs[0].device) for _ in coefs]
    n = len(coefs)
    for c in coefs:
        _need(c, torch.int32, "coef")
        assert c.shape == coefs[0].shape
    px = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    cf = (ctypes.c_void_p * n)(*[c.data_ptr() for c in coefs])
    lv = (ctypes.c_int * n)(*[int(v) for v in leaf_bs])
    _check(lib().odhip_inverse_levels(px, w, h * w, cf, lv, n, nplanes, w, h, int(dec),
                                      int(pic_w), int(pic_h), _stream()), "odhip_inverse_levels")
    return outs


def cfl_refs_from_luma(luma_jobs, refs=None, copies=2):
    """Chroma-from-luma reference planes from the luma band stage's chosen candidates
    (od_resample_luma_coeffs, non-TF branch): luma_jobs[j] at level bs >= 1 -> refs[j]
    int32 [copies*nplanes, h/2, w/2] for the chroma level bs - 1."""
    import torch
    if refs is None:
        refs = []
        for j in luma_jobs:
            nplanes, h, w = j.coef.shape
            refs.append(torch.empty((copies * nplanes, h // 2, w // 2), dtype=torch.int32,
                                    device=j.coef.device))
    ptrs = (ctypes.c_void_p * len(refs))(*[r.data_ptr() for r in refs])
    _check(lib().odhip_cfl_refs_from_luma(_jobs_array(luma_jobs), len(luma_jobs), ptrs, int(copies),
                                          _stream()), "odhip_cfl_refs_from_luma")
    return refs


def pvq_ref_set_context(ctx):
    """Selects which of the two library contexts the following pvq_ref_* calls of this
    thread use (one call sequence may be in flight per context)."""
    _check(lib().odhip_pvq_ref_set_context(int(ctx)), "odhip_pvq_ref_set_context")
    # the test hooks are per context: a test that set a margin / perturbation / tolerance scale and
    # then switches context would silently run without them
    if any(_hooks[k] != v for k, v in (("margin", 0.0), ("perturb", 0), ("tol", 1.0))):
        _apply_hooks()


def pvq_ref_choose_multi(jobs, pvq_norm_lambda):
    """The with-reference stage's choice alone (choice records incl. the synthesis
    parameters), for inverse_levels_pvq_ref."""
    _check(lib().odhip_pvq_ref_choose_multi(_refjobs_array(jobs), len(jobs), pvq_norm_lambda, _stream()),
           "odhip_pvq_ref_choose_multi")


def pvq_ref_choose_priced_multi(jobs, pvq_norm_lambda, fused_bands=False):
    """The with-reference stage's choice priced on the device.  fused_bands=False: after
    pvq_ref_bands_multi, every band decided from its candidate records
    (odhip_pvq_ref_choose_priced_multi); True: band stage with the per-lane bands decided
    inside their searches, then the rest (odhip_pvq_ref_bands_priced_multi +
    odhip_pvq_ref_resolve + odhip_pvq_ref_choose_priced_rest_multi).  Followed by the host-libm
    resolve; returns the number of bands it re-decided."""
    arr = _refjobs_array(jobs)
    L = lib()
    if fused_bands:
        _check(L.odhip_pvq_ref_bands_priced_multi(arr, len(jobs), pvq_norm_lambda, _stream()),
               "odhip_pvq_ref_bands_priced_multi")
        if _resolved(L.odhip_pvq_ref_resolve(arr, len(jobs), pvq_norm_lambda, _stream()), "odhip_pvq_ref_resolve"):
            # bands were re-run with the host's theta: everything is decided from the records
            _check(L.odhip_pvq_ref_choose_priced_multi(arr, len(jobs), pvq_norm_lambda, _stream()),
                   "odhip_pvq_ref_choose_priced_multi")
        else:
            _check(L.odhip_pvq_ref_choose_priced_rest_multi(arr, len(jobs), pvq_norm_lambda, _stream()),
                   "odhip_pvq_ref_choose_priced_rest_multi")
    else:
        _check(L.odhip_pvq_ref_choose_priced_multi(arr, len(jobs), pvq_norm_lambda, _stream()),
               "odhip_pvq_ref_choose_priced_multi")
    return _resolved(L.odhip_pvq_ref_choose_priced_resolve(arr, len(jobs), pvq_norm_lambda, _stream()),
                     "odhip_pvq_ref_choose_priced_resolve")


def pvq_decode_bands(ref, y, sym, qm, qm_inv, q0, beta, is_keyframe, pli):
    """The decoder's arithmetic for a batch of bands (odhip_pvq_decode_bands): ref, y int32
    [nbands, n] CUDA, sym int32 [nbands, 4] = {gain symbol as read, itheta, noref, 0}, qm /
    qm_inv int16 [n].  Returns (out int32 [nbands, n], info int32 [nbands, 2] = {K, skip})."""
    import torch
    _need(ref, torch.int32, "ref")
    _need(y, torch.int32, "y")
    _need(sym, torch.int32, "sym")
    _need(qm, torch.int16, "qm")
    _need(qm_inv, torch.int16, "qm_inv")
    nbands, n = ref.shape
    assert y.shape == ref.shape and sym.shape == (nbands, 4)
    out = torch.empty_like(ref)
    info = torch.empty((nbands, 2), dtype=torch.int32, device=ref.device)
    _check(lib().odhip_pvq_decode_bands(_p(out), _p(ref), _p(y), int(n), nbands, _p(sym),
                                        _p(qm), _p(qm_inv), int(q0), int(beta), int(is_keyframe), int(pli),
                                        _p(info), _stream()), "odhip_pvq_decode_bands")
    return out, info


def pvq_ref_bands_decided_multi(jobs, pvq_norm_lambda):
    """The with-reference band stage with the priced choice of every band made inside its
    search (odhip_pvq_ref_bands_decided_multi), followed by the two resolves.  Leaves the
    choice records and, in slot 0 of each job's y, the winners' pulse vectors.  Returns
    (bands re-run with the host's theta, bands re-decided with the host libm)."""
    arr = _refjobs_array(jobs)
    L = lib()
    _check(L.odhip_pvq_ref_bands_decided_multi(arr, len(jobs), pvq_norm_lambda, _stream()),
           "odhip_pvq_ref_bands_decided_multi")
    n = _resolved(L.odhip_pvq_ref_resolve_finish(arr, len(jobs), pvq_norm_lambda, _stream()),
                  "odhip_pvq_ref_resolve_finish")
    m = _resolved(L.odhip_pvq_ref_choose_priced_resolve(arr, len(jobs), pvq_norm_lambda, _stream()),
                  "odhip_pvq_ref_choose_priced_resolve")
    return n, m


def inverse_levels_pvq_ref(jobs, dec, pic_w, pic_h, outs=None):
    """Inverse of several partition levels of one plane set fed by the with-reference
    band stage: dequantise-on-load from the chosen candidates (no dequantised plane)."""
    import torch
    nplanes, h, w = jobs[0].coef.shape
    if outs is None:
        outs = [torch.empty((nplanes, h, w), dtype=px_dtype(), device=jobs[0].coef.device)
                for _ in jobs]
    px = (ctypes.c_void_p * len(jobs))(*[o.data_ptr() for o in outs])
    _check(lib().odhip_inverse_levels_pvq_ref(px, w, h * w, _refjobs_array(jobs), len(jobs), int(dec), int(pic_w),
                                              int(pic_h), _stream()), "odhip_inverse_levels_pvq_ref")
    return outs


# ---- contexts ------------------------------------------------------------------------
class Context:
    """odhip_ctx: owner of the library state one call sequence needs (daala_hip.h).
    `with ctx:` makes it the calling thread's current context."""

    def __init__(self, device=0):
        self.handle = lib().odhip_create(int(device))
        if not self.handle:
            raise DaalaHipError("odhip_create(%d) failed" % device)
        self._prev = []

    def __enter__(self):
        self._prev.append(lib().odhip_get_current())
        _check(lib().odhip_make_current(self.handle), "odhip_make_current")
        if any(_hooks[k] != v for k, v in (("margin", 0.0), ("perturb", 0), ("tol", 1.0))):
            _apply_hooks()      # per-context test hooks follow the selection
        return self

    def __exit__(self, *exc):
        _check(lib().odhip_make_current(self._prev.pop()), "odhip_make_current")

    def set_fpr(self, on=True):
        """Full-precision references: picture planes of this context's calls are int16
        samples at 12 bits (odhip_ctx_set_fpr)."""
        _check(lib().odhip_ctx_set_fpr(self.handle, int(bool(on))), "odhip_ctx_set_fpr")
        return self

    def destroy(self):
        if self.handle:
            lib().odhip_destroy(self.handle)
            self.handle = None


# ---- odhip_pipe: the frame-batch step as one C call -----------------------------------
PIPE_STAGES = ("image_copy_pad_luma", "forward_pyramid_luma", "pvq_noref_bands", "pvq_choose",
               "cfl_refs_from_luma", "dequant_inverse_luma", "image_copy_pad_chroma",
               "forward_pyramid_chroma", "pvq_ref_bands", "pvq_ref_choose", "dequant_inverse_chroma")
(BUF_PIC, BUF_PX, BUF_LEVEL, BUF_RECON, BUF_BAND, BUF_Y, BUF_CHOICE, BUF_ITEMS, BUF_REF,
 BUF_RATE) = range(10)
BUF_PRED = 10     # inter mode: the coded-size prediction planes


_PipeConfig, _ExportSection, _ExportLayout = _S["odhip_pipe_config"], _S["odhip_export_section"], _S["odhip_export_layout"]


def export_layout_make(nblocks, bs, with_ref):
    """odhip_export_layout_make for sections of nblocks[i] blocks at level bs[i] -> (ctypes layout, dict)."""
    lay = _ExportLayout()
    n = len(bs)
    _check(lib().odhip_export_layout_make(ctypes.byref(lay), n, (ctypes.c_long * n)(*nblocks), (ctypes.c_int * n)(*bs),
                                          (ctypes.c_int * n)(*[int(bool(w)) for w in with_ref])),
           "odhip_export_layout_make")
    return lay, _layout_dict(lay)


def _layout_dict(lay):
    secs = [{k: int(getattr(lay.section[i], k)) for k in ("bs", "ngroups", "cap_words", "blocks_per_group", "record_bytes",
                                                         "nrecords", "records_off", "group_base_off", "stream_off")}
            for i in range(lay.nsections)]
    return {"nsections": int(lay.nsections), "fixed_bytes": int(lay.fixed_bytes),
            "total_bytes": int(lay.total_bytes), "sections": secs}


def decode_export_sections(host, lay):
    """Reference-side decoder of the export format (include/daala_hip.h, export_kernels.hip): `host` = the buffer
    as numpy uint8, `lay` = the layout dict.  Per section (y int32 [B][len], band int32 [B][nb][4] = {coded gain
    index, itheta, max_theta, k}, coded bool [B][nb]).  A host entropy coder walks the same records and words
    sequentially; this vectorised form exists for the tests and the bench.  k of a band that is not coded is 0."""
    hdr = host[:128].view(np.uint32)
    out = []
    rec4, rec8 = np.dtype(_S["odhip_export_record4"]), np.dtype(_S["odhip_export_record8"])
    for si, sec in enumerate(lay["sections"]):
        nb, offs, ln = pvq_band_layout(sec["bs"])
        G = sec["blocks_per_group"] * nb          # records per group
        B = sec["nrecords"] // nb
        assert int(hdr[16 + si]) == 0, "export stream of section %d overflowed" % si
        rb = sec["record_bytes"]
        rec = host[sec["records_off"]:sec["records_off"] + sec["nrecords"] * rb].view(rec8 if rb == 8 else rec4)
        gbase = host[sec["group_base_off"]:sec["group_base_off"] + sec["ngroups"] * 4].view(np.uint32).astype(np.int64)
        total = int(hdr[si])
        words = host[sec["stream_off"]:sec["stream_off"] + total * 2].view(np.uint16)
        nw = (rec["fn"] & 0x1ff).astype(np.int64)
        assert total == int(nw.sum()), (si, total, int(nw.sum()))
        # first word of every band: its group's base + the words of the group's earlier bands
        pad = (-len(nw)) % G
        nwp = np.concatenate([nw, np.zeros(pad, np.int64)]).reshape(-1, G)
        start = (gbase[:, None] + np.cumsum(nwp, axis=1) - nwp).reshape(-1)[:len(nw)]
        band_of_word = np.repeat(np.arange(len(nw)), nw)
        rank = np.arange(len(band_of_word)) - np.repeat(np.cumsum(nw) - nw, nw)
        w = words[start[band_of_word] + rank].astype(np.int64)
        pos = w & 127
        val = ((w >> 7) ^ 256) - 256          # sign-extend the 9-bit count
        keep = np.ones(len(w), bool)
        idx = np.nonzero(val == -256)[0]
        # escapes: the word after a count of -256 is the count itself.  (A payload word can look like an escape:
        # walk them in order so that a payload is never taken for one.)
        if len(idx):
            is_payload = np.zeros(len(w), bool)
            for i in idx:
                if is_payload[i]:
                    continue
                is_payload[i + 1] = True
                full = int(w[i + 1])
                val[i] = full - 65536 if full >= 32768 else full
            keep = ~is_payload
        y = np.zeros((B, ln), np.int32)
        bw = band_of_word[keep]
        y[bw // nb, np.asarray(offs)[bw % nb] + pos[keep]] = val[keep]
        band = np.zeros((B, nb, 4), np.int32)
        r = rec.reshape(B, nb)
        band[..., 0] = r["qg"]
        band[..., 1] = r["itheta"] if rb == 8 else -1
        band[..., 2] = r["max_theta"] if rb == 8 else 0
        # K of a coded band = the magnitudes of its counts (not exported)
        for i in range(nb):
            band[:, i, 3] = np.abs(y[:, offs[i]:offs[i + 1]]).sum(axis=1)
        coded = ((r["fn"] >> 10) & 3) == 0
        out.append((y, band, coded))
    return out


class Pipe:
    """ctypes mirror of odhip_pipe (include/daala_hip.h): F resident 4:2:0 (chroma_444=True:
    4:4:4) pictures, one C call per step.  Buffers are read / written as numpy arrays."""

    def __init__(self, quant, frames, pic_w, pic_h, chroma_cfl=True, serial=False, device=0,
                 pvq_norm_lambda=0.147, price=False, fpr_bits=0, inter=False, chroma_444=False):
        """price=True: the choices price every candidate with od_pvq_rate's closed form on
        the device (odhip_pvq_*choose_priced_*), nothing for the host to do in a step.
        fpr_bits = 8 / 10 / 12: full-precision references, pictures of that bit depth (uint8 /
        int16), coded planes and reconstructions int16 at 12 bits.  chroma_444=True: chroma planes
        of the picture size at 5 levels (chroma_levels), odd sizes accepted."""
        L = lib()
        cfg = _PipeConfig(device=int(device), frames=int(frames), pic_w=int(pic_w), pic_h=int(pic_h),
                          chroma_cfl=int(bool(chroma_cfl)), serial=int(bool(serial)), price=int(bool(price)),
                          fpr_bits=int(fpr_bits), inter=int(bool(inter)), chroma_444=int(bool(chroma_444)),
                          pvq_norm_lambda=float(pvq_norm_lambda), quant=ctypes.addressof(quant.c))
        self.h = L.odhip_pipe_create(ctypes.byref(cfg))
        if not self.h:
            raise DaalaHipError("odhip_pipe_create failed")
        self.frames, self.pic_w, self.pic_h = int(frames), int(pic_w), int(pic_h)
        self.W, self.H = (pic_w + 63) & ~63, (pic_h + 63) & ~63
        self.chroma_cfl = bool(chroma_cfl)
        self.fpr_bits = int(fpr_bits)
        self.inter = bool(inter)
        self.chroma_444 = bool(chroma_444)
        cdec = 0 if chroma_444 else 1
        # the chroma pictures: [2F][ch][cw] (all Cb, then all Cr)
        self.cw, self.ch = (self.pic_w + cdec) >> cdec, (self.pic_h + cdec) >> cdec
        self.chroma_levels = int(L.odhip_pipe_chroma_levels(self._p()))
        # test hooks the tests asked for (module state above) reach this pipe's contexts too
        global _pipes
        if _pipes is None:
            import weakref
            _pipes = weakref.WeakSet()
        _pipes.add(self)
        if _hooks["margin"] > 0 or _hooks["perturb"] or _hooks["tol"] != 1.0:
            _check(L.odhip_pipe_set_test_hooks(self._p(), _hooks["margin"], int(_hooks["perturb"]), _hooks["tol"]),
                   "odhip_pipe_set_test_hooks")

    def _p(self):
        return ctypes.c_void_p(self.h)

    def destroy(self):
        if self.h:
            lib().odhip_pipe_destroy(self._p())
            self.h = None

    def set_pictures(self, luma, chroma):
        """luma uint8 [F, pic_h, pic_w], chroma uint8 [2F, pic_h/2, pic_w/2] (chroma_444: [2F,
        pic_h, pic_w]; all Cb, then all Cr): numpy arrays (uploaded) or CUDA tensors (device copy)."""
        dev = hasattr(luma, "data_ptr")
        dt = np.int16 if self.fpr_bits > 8 else np.uint8
        if not dev:
            luma = np.ascontiguousarray(luma, dt)         # kept alive until the call returns
            chroma = np.ascontiguousarray(chroma, dt)
        pl = luma.data_ptr() if dev else luma.ctypes.data
        pc = chroma.data_ptr() if dev else chroma.ctypes.data
        assert tuple(luma.shape) == (self.frames, self.pic_h, self.pic_w)
        assert tuple(chroma.shape) == (2 * self.frames, self.ch, self.cw)
        _check(lib().odhip_pipe_set_pictures(self._p(), ctypes.c_void_p(pl), ctypes.c_void_p(pc),
                                             int(dev)), "odhip_pipe_set_pictures")

    def set_reference_pictures(self, luma, chroma):
        """Inter mode: the prediction pictures of the batch (numpy, same shapes and depth as
        set_pictures)."""
        dt = np.int16 if self.fpr_bits > 8 else np.uint8
        luma = np.ascontiguousarray(luma, dt)
        chroma = np.ascontiguousarray(chroma, dt)
        assert tuple(luma.shape) == (self.frames, self.pic_h, self.pic_w)
        assert tuple(chroma.shape) == (2 * self.frames, self.ch, self.cw)
        _check(lib().odhip_pipe_set_reference_pictures(self._p(), ctypes.c_void_p(luma.ctypes.data),
                                                       ctypes.c_void_p(chroma.ctypes.data), 0),
               "odhip_pipe_set_reference_pictures")

    def _mc_frames(self, luma, chroma, host_only):
        # lists (one entry per slot) of [F][H][W] / [2F][H >> cdec][W >> cdec] planes in the planes' sample type
        dt = np.int16 if self.fpr_bits else np.uint8
        cdec = 0 if self.chroma_444 else 1
        shapes = ((self.frames, self.H, self.W), (2 * self.frames, self.H >> cdec, self.W >> cdec))
        n = len(luma)
        if not (1 <= n <= 3 and len(chroma) == n):
            raise DaalaHipError("reference frames: 1..3 slots, luma and chroma lists of the same length")
        ptrs, keep, dev = ([], []), [], None
        for i, group in enumerate((luma, chroma)):
            for t in group:
                if hasattr(t, "data_ptr"):
                    is_dev = bool(t.is_cuda)
                    ok = t.is_contiguous() and tuple(t.shape) == shapes[i] and t.element_size() == np.dtype(dt).itemsize
                    ptr = t.data_ptr()
                else:
                    is_dev = False
                    t = np.ascontiguousarray(t, dt)
                    ok = t.shape == shapes[i]
                    ptr = t.ctypes.data
                if not ok or (dev is not None and dev != is_dev) or (host_only and is_dev):
                    raise DaalaHipError("reference frames: contiguous planes %s / %s of %s, all on one side"
                                        % (shapes[0], shapes[1], np.dtype(dt).name))
                dev = is_dev
                keep.append(t)
                ptrs[i].append(ptr)
        return (ctypes.c_void_p * n)(*ptrs[0]), (ctypes.c_void_p * n)(*ptrs[1]), n, int(dev), keep

    def set_reference_frames(self, luma, chroma):
        """Inter mode: the resident reference frames the steps predict from (odhip_pipe_set_reference_frames): lists
        with one entry per slot (1..3) of coded-size planes, luma [F][H][W], chroma [2F][H >> cdec][W >> cdec], uint8 -
        with fpr_bits int16 at 12 bits -, numpy arrays or CUDA tensors.  None / []: drop frames and grids."""
        if not luma:
            _check(lib().odhip_pipe_set_reference_frames(self._p(), 0, None, None, 0),
                   "odhip_pipe_set_reference_frames")
            return
        pl, pc, n, dev, keep = self._mc_frames(list(luma), list(chroma), False)
        _check(lib().odhip_pipe_set_reference_frames(self._p(), n, pl, pc, dev), "odhip_pipe_set_reference_frames")

    def _mc_call(self, fn, name, grid):
        g = _mc_grid(grid, self.W, self.H)
        if g.shape[0] != self.frames:
            raise DaalaHipError("%s: one grid per picture" % name)
        rc = fn(self._p(), g.ctypes.data_as(ctypes.c_void_p))
        if rc == ERANGE:
            raise MotionRangeError("%s: a vector is outside the legal range" % name)
        _check(rc, name)
        return g

    def set_mvs(self, grid):
        """The resident grids (MV_POINT [F][H/8 + 1][W/8 + 1]); from now on every inter step builds its prediction
        from the reference frames and these.  None: no grid (set_reference_pictures supplies the prediction)."""
        if grid is None:
            _check(lib().odhip_pipe_set_mvs(self._p(), None), "odhip_pipe_set_mvs")
        else:
            self._mc_call(lib().odhip_pipe_set_mvs, "odhip_pipe_set_mvs", grid)

    def feed_reference_frames(self, luma, chroma):
        """The reference frames of the NEXT step from host memory (pinned CPU torch tensors: asynchronous; or numpy),
        same lists as set_reference_frames; kept alive here until the next feed_reference_frames or destroy - sync()
        before reusing pinned buffers."""
        pl, pc, n, _, keep = self._mc_frames(list(luma), list(chroma), True)
        _check(lib().odhip_pipe_feed_reference_frames(self._p(), pl, pc), "odhip_pipe_feed_reference_frames")
        self._mc_keep_frames = getattr(self, "_mc_keep_frames", [])[-1:] + [keep]

    def feed_mvs(self, grid):
        """The grids of the NEXT step (numpy MV_POINT, or a pinned CPU uint8 torch tensor's numpy view): checked
        (MotionRangeError), then copied on the copy stream; the last two fed arrays are kept alive here."""
        g = self._mc_call(lib().odhip_pipe_feed_mvs, "odhip_pipe_feed_mvs", grid)
        self._mc_keep_grids = getattr(self, "_mc_keep_grids", [])[-1:] + [g]

    def set_motion_search(self, log_size, rng, res=0, lam=0):
        """Every inter step searches its own grids (odhip_pipe_set_motion_search: uniform spacing 8 << log_size,
        full-pel range `rng`, sub-pel resolution res 0 (1/8 pel) .. 3 (none), vector weight `lam`) from its pictures
        and the luma reference frames; set_mvs / feed_mvs are refused while it is on.  rng < 0: off."""
        _check(lib().odhip_pipe_set_motion_search(self._p(), int(log_size), int(rng), int(res), int(lam)),
               "odhip_pipe_set_motion_search")

    def set_motion_search2(self, log_size, rng, res=0, lam=0, lam_subpel=None, flags=0):
        """odhip_pipe_set_motion_search2: the search with ME_CHROMA / ME_SATD in `flags` and the sub-pel stage's own
        lambda (default: lam).  rng < 0 switches the search off."""
        lam_subpel = lam if lam_subpel is None else lam_subpel
        _check(lib().odhip_pipe_set_motion_search2(self._p(), int(log_size), int(rng), int(res), int(lam),
                                                   int(lam_subpel), int(flags)), "odhip_pipe_set_motion_search2")

    def set_motion_search3(self, log_size, rng, res=0, lam=0, lam_subpel=None, flags=0, levels=0, refine=2):
        """odhip_pipe_set_motion_search3: the search coarse to fine over `levels` (0..2) halvings - `rng` is the radius
        at the top level, `refine` (1..8) at every level below; levels = 0 is set_motion_search2."""
        lam_subpel = lam if lam_subpel is None else lam_subpel
        _check(lib().odhip_pipe_set_motion_search3(self._p(), int(log_size), int(rng), int(res), int(lam),
                                                   int(lam_subpel), int(flags), int(levels), int(refine)),
               "odhip_pipe_set_motion_search3")

    def set_motion_search_vbs(self, log_min, log_max, rng, res=0, lam=0, lam_subpel=None, flags=0, levels=0, refine=2,
                              split_penalty=0):
        """odhip_pipe_set_motion_search_vbs: every inter step searches a grid of mixed block sizes, 8 << log_min to
        8 << log_max - a cell splits where the smaller size's prediction is better by more than split_penalty/8 in
        SAD; log_min == log_max is set_motion_search3 at that size.  rng < 0 switches the search off."""
        lam_subpel = lam if lam_subpel is None else lam_subpel
        _check(lib().odhip_pipe_set_motion_search_vbs(self._p(), int(log_min), int(log_max), int(rng), int(res),
                                                      int(lam), int(lam_subpel), int(flags), int(levels), int(refine),
                                                      int(split_penalty)), "odhip_pipe_set_motion_search_vbs")

    def read_mvs(self, want_cost=False):
        """The grids of the last enqueued step (odhip_pipe_mvs_read; syncs): MV_POINT [F][H/8 + 1][W/8 + 1], with
        want_cost (the search is on) also the winners' costs as uint32 of the same shape."""
        shape = (self.frames, self.H // 8 + 1, self.W // 8 + 1)
        grid = np.zeros(shape, MV_POINT)
        cost = np.zeros(shape, np.uint32) if want_cost else None
        _check(lib().odhip_pipe_mvs_read(self._p(), grid.ctypes.data_as(ctypes.c_void_p),
                                         cost.ctypes.data_as(ctypes.c_void_p) if want_cost else None),
               "odhip_pipe_mvs_read")
        return (grid, cost) if want_cost else grid

    def feed(self, luma, chroma):
        """The pictures of the NEXT step from host memory, copied while the enqueued steps
        compute (odhip_pipe_feed).  luma / chroma: pinned CPU torch tensors (asynchronous) or
        numpy arrays, same shapes as set_pictures; the caller keeps them alive and untouched
        until sync()."""
        dt = np.int16 if self.fpr_bits > 8 else np.uint8
        if hasattr(luma, "data_ptr"):
            assert not luma.is_cuda and luma.is_contiguous() and chroma.is_contiguous()
            pl, pc = luma.data_ptr(), chroma.data_ptr()
        else:
            assert luma.dtype == dt and chroma.dtype == dt and luma.flags["C_CONTIGUOUS"]
            pl, pc = luma.ctypes.data, chroma.ctypes.data
        assert tuple(luma.shape) == (self.frames, self.pic_h, self.pic_w)
        assert tuple(chroma.shape) == (2 * self.frames, self.ch, self.cw)
        _check(lib().odhip_pipe_feed(self._p(), ctypes.c_void_p(pl), ctypes.c_void_p(pc)), "odhip_pipe_feed")

    def export_bytes(self):
        """Bytes one step copies to the host with set_export (odhip_pipe_export_bytes)."""
        return int(lib().odhip_pipe_export_bytes(self._p()))

    def set_export(self, host):
        """host: a pinned CPU uint8 torch tensor of export_bytes() bytes (kept alive by the caller
        until set_export(None)), or None to stop: every following step leaves the record and the pulses of
        every band there, compacted on the device (odhip_pipe_set_export; decode_export reads it back)."""
        if host is None:
            _check(lib().odhip_pipe_set_export(self._p(), ctypes.c_void_p(0)), "odhip_pipe_set_export")
            return
        assert not host.is_cuda and host.is_contiguous() and host.numel() * host.element_size() >= self.export_bytes()
        _check(lib().odhip_pipe_set_export(self._p(), ctypes.c_void_p(host.data_ptr())), "odhip_pipe_set_export")

    def set_export_ring(self, slots):
        """slots: a list of n >= 2 pinned CPU uint8 torch tensors of export_bytes() bytes each (kept alive by the pipe
        until the ring is stopped), or None / [] to stop (the pipe is synced, steps nobody took are dropped).  Step s
        from now on lands in slots[s % n] (odhip_pipe_set_export_ring); export_take / export_release hand them out."""
        L = lib()
        if not slots:
            _check(L.odhip_pipe_set_export_ring(self._p(), None, 0), "odhip_pipe_set_export_ring")
            self._ring = None
            return
        slots = list(slots)
        for t in slots:
            assert not t.is_cuda and t.is_contiguous() and t.numel() * t.element_size() >= self.export_bytes()
        ptrs = (ctypes.c_void_p * len(slots))(*[t.data_ptr() for t in slots])
        _check(L.odhip_pipe_set_export_ring(self._p(), ptrs, len(slots)), "odhip_pipe_set_export_ring")
        self._ring = slots

    def export_take(self, wait=True):
        """The oldest complete step not taken yet: (step, numpy uint8 view of its slot, overflow mask) - the view is
        valid until export_release(step) - or None when there is none (wait=True blocks only for a step whose copies
        are enqueued: step again or flush() first)."""
        L = lib()
        step = ctypes.c_long()
        buf = ctypes.c_void_p()
        ovf = ctypes.c_uint32()
        rc = L.odhip_pipe_export_take(self._p(), int(bool(wait)), ctypes.byref(step), ctypes.byref(buf),
                                      ctypes.byref(ovf))
        if rc < 0:
            _check(rc, "odhip_pipe_export_take")
        if rc == 0:
            return None
        slot = self._ring[step.value % len(self._ring)]
        assert slot.data_ptr() == buf.value
        return step.value, slot.numpy(), int(ovf.value)

    def export_release(self, step):
        """Gives the slot of `step` (the oldest taken, not released step) back to the pipe."""
        _check(lib().odhip_pipe_export_release(self._p(), int(step)), "odhip_pipe_export_release")

    def export_layout(self):
        """odhip_pipe_export_layout as a dict: nsections, fixed_bytes, total_bytes, sections[] of
        {bs, ngroups, cap_words, nrecords, records_off, group_base_off, stream_off}."""
        lay = _ExportLayout()
        _check(lib().odhip_pipe_export_layout(self._p(), ctypes.byref(lay)), "odhip_pipe_export_layout")
        return _layout_dict(lay)

    def export_stale(self):
        return int(lib().odhip_pipe_export_stale(self._p()))

    def export_shipped_bytes(self, host):
        """Bytes of the export buffer `host` (numpy uint8 view) that crossed the bus for the step it holds: the
        fixed part plus the used prefix of every stream (rounded up to the 16-byte vectors the ship kernel
        moves)."""
        lay = self.export_layout()
        totals = host[:64].view(np.uint32)
        n = lay["fixed_bytes"]
        for i, sec in enumerate(lay["sections"]):
            n += (min(int(totals[i]), sec["cap_words"]) * 2 + 15) // 16 * 16
        return n

    def decode_export(self, host):
        """The export buffer `host` (numpy uint8) decoded back to what tests/_pipeline_check.gpu_decisions reads from
        the dense device buffers: {(set, level): (y int32 [B][len], band int32 [B][nb][4] = {coded gain index,
        itheta, max_theta, k}, coded bool [B][nb])}."""
        secs = decode_export_sections(host, self.export_layout())
        return {((0, i) if i < 5 else (1, i - 5)): v for i, v in enumerate(secs)}

    def set_quants(self, quants):
        """Picture f of every following step coded at quants[f]: a list of `frames` QuantTables with the
        pipe's use_masking and hvs_qm (quantizer / base_quantizer free), or None for the pipe's own quant
        again (odhip_pipe_set_quants).  Steps already enqueued keep the quantisers they were enqueued with."""
        if quants is None:
            _check(lib().odhip_pipe_set_quants(self._p(), None, 0), "odhip_pipe_set_quants")
            self._quants = None
            return
        quants = list(quants)
        ptrs = (ctypes.c_void_p * max(1, len(quants)))(
            *[None if q is None else ctypes.cast(ctypes.byref(q.c), ctypes.c_void_p) for q in quants])
        _check(lib().odhip_pipe_set_quants(self._p(), ptrs, len(quants)), "odhip_pipe_set_quants")
        self._quants = quants        # (the library copies them; kept for the caller's inspection)

    def step(self):
        _check(lib().odhip_pipe_step(self._p()), "odhip_pipe_step")

    def flush(self):
        _check(lib().odhip_pipe_flush(self._p()), "odhip_pipe_flush")

    def sync(self):
        _check(lib().odhip_pipe_sync(self._p()), "odhip_pipe_sync")

    def k_range(self):
        """Bands above ODHIP_PVQ_MAX_K counted at this pipe's syncs so far."""
        return int(lib().odhip_pipe_k_range(self._p()))

    def stage(self, name, parity=0):
        _check(lib().odhip_pipe_stage(self._p(), PIPE_STAGES.index(name), int(parity)),
               "odhip_pipe_stage(%s)" % name)

    def buffer(self, what, set_, level=0, parity=-1):
        ptr = ctypes.c_void_p()
        n = ctypes.c_size_t()
        _check(lib().odhip_pipe_buffer(self._p(), int(what), int(set_), int(level), int(parity),
                                       ctypes.byref(ptr), ctypes.byref(n)), "odhip_pipe_buffer")
        return ptr.value, n.value

    def read(self, what, set_, level=0, parity=-1, dtype=np.uint8):
        """parity -1: the buffers of the last step() (0 when the pipe is driven stage by stage)."""
        ptr, n = self.buffer(what, set_, level, parity)
        out = np.empty(n, np.uint8)
        _check(lib().odhip_pipe_read(self._p(), out.ctypes.data_as(ctypes.c_void_p),
                                     ctypes.c_void_p(ptr), n), "odhip_pipe_read")
        return out.view(dtype)

    def write(self, what, set_, level, data, parity=-1):
        ptr, n = self.buffer(what, set_, level, parity)
        data = np.ascontiguousarray(data)
        assert data.nbytes == n, (data.nbytes, n)
        _check(lib().odhip_pipe_write(self._p(), ctypes.c_void_p(ptr), data.ctypes.data_as(ctypes.c_void_p), n),
               "odhip_pipe_write")

    def record(self, enable):
        _check(lib().odhip_pipe_record(self._p(), int(bool(enable))), "odhip_pipe_record")

    def timings(self):
        """{stage: (average ms per launch group, groups)} of the recorded steps."""
        ms = (ctypes.c_double * len(PIPE_STAGES))()
        cnt = (ctypes.c_int * len(PIPE_STAGES))()
        _check(lib().odhip_pipe_timings(self._p(), ms, cnt), "odhip_pipe_timings")
        return {PIPE_STAGES[i]: (ms[i], cnt[i]) for i in range(len(PIPE_STAGES)) if cnt[i]}

    def search_timings(self, chroma, max_n=256):
        buf = (ctypes.c_float * max_n)()
        n = lib().odhip_pipe_search_timings(self._p(), int(bool(chroma)), buf, max_n)
        if n < 0:
            raise DaalaHipError("odhip_pipe_search_timings failed with code %d" % n)
        return [buf[i] for i in range(n)]

    def time_pyramid(self, n=10):
        ms = ctypes.c_double()
        _check(lib().odhip_pipe_time_pyramid(self._p(), int(n), ctypes.byref(ms)),
               "odhip_pipe_time_pyramid")
        return ms.value

    def time_stage(self, stage, n=10, parity=-1):
        """Average ms per launch group of one filter + DCT stage (a PIPE_STAGES name) run alone."""
        ms = ctypes.c_double()
        _check(lib().odhip_pipe_time_stage(self._p(), PIPE_STAGES.index(stage), int(parity), int(n),
                                           ctypes.byref(ms)), "odhip_pipe_time_stage")
        return ms.value

    def host_wait_ms(self):
        return float(lib().odhip_pipe_host_wait_ms(self._p()))

    def theta_reruns(self):
        return int(lib().odhip_pipe_theta_reruns(self._p()))

    def theta_listed(self):
        """Bands found inside the margin of the device acos so far (theta recomputed by the host's libm)."""
        return int(lib().odhip_pipe_theta_listed(self._p()))

    def price_reruns(self):
        """Priced choices re-decided with the host libm so far (price=True pipes)."""
        return int(lib().odhip_pipe_price_reruns(self._p()))

    def set_metrics(self, sse=True, psnrhvs=True, depth=2, **optional):
        """Every following step measures every picture, plane and partition level against its source on the device
        (odhip_pipe_set_metrics5): SSE and / or PSNR-HVS-M and / or, each False unless given, the columns of
        PIPE_METRIC_COLUMNS - ssim, msssim, fastssim, and ciede (CIEDE2000 of every picture and luma level) - into a
        ring of `depth` slots, taken with metrics_take.  All False stops (the pipe is synced, untaken steps are
        dropped)."""
        flags = (METRIC_SSE if sse else 0) | (METRIC_PSNRHVS if psnrhvs else 0)
        for name, flag, _, _ in PIPE_METRIC_COLUMNS:
            flags |= flag if optional.pop(name, False) else 0
        if optional:
            raise TypeError("set_metrics: no metric named %s" % ", ".join(sorted(optional)))
        _check(lib().odhip_pipe_set_metrics5(self._p(), flags, int(depth)), "odhip_pipe_set_metrics5")

    def metrics_layout(self):
        info = _PipeMetricsInfo()
        _check(lib().odhip_pipe_metrics_layout(self._p(), ctypes.byref(info)), "odhip_pipe_metrics_layout")
        return info


    def metrics_take(self, wait=True):
        """The oldest complete step's metrics (PipeMetrics), or None when none is complete (wait=True blocks only for a
        step whose copy is enqueued: step again or flush() first).  Taking frees its ring slot."""
        info = self.metrics_layout()
        step = ctypes.c_long()
        # take5's arrays in its order: sse, hvs, then every optional column the slot has (None: skipped)
        cols = [np.zeros(info.values, np.int64), np.zeros(info.values, np.float64)]
        for _, flag, tail, _ in PIPE_METRIC_COLUMNS:
            shape = self.metrics_ciede_values() if tail is None else (info.values,) + tail
            cols.append(np.zeros(shape, np.float64) if info.flags & flag else None)
        rc = lib().odhip_pipe_metrics_take5(self._p(), int(bool(wait)), ctypes.byref(step),
                                            *[None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in cols])
        if rc < 0:
            _check(rc, "odhip_pipe_metrics_take5")
        if rc == 0:
            return None
        npix = (ctypes.c_long * 2)()
        nwin = (ctypes.c_long * 2)()
        _check(lib().odhip_pipe_metrics_counts(self._p(), npix, nwin), "odhip_pipe_metrics_counts")
        m = PipeMetrics(step.value, cols[0], cols[1], info, npix[:], nwin[:])
        for (name, _, _, needs), a in zip(PIPE_METRIC_COLUMNS, cols[2:]):
            if a is not None:
                getattr(m, "set_" + name)(a, needs(self))
        return m

    def metrics_ciede_values(self):
        """Entries of the CIEDE2000 column of a step (odhip_pipe_metrics_ciede_values): 5F."""
        n = lib().odhip_pipe_metrics_ciede_values(self._p())
        if n < 0:
            _check(n, "odhip_pipe_metrics_ciede_values")
        return int(n)

    def metrics_msssim_weights(self):
        """The five MS-SSIM weights of a plane of (luma, chroma) (odhip_pipe_metrics_msssim_weights): int64 [2][5]."""
        wt = (ctypes.c_int64 * (2 * MSSSIM_SCALES))()
        _check(lib().odhip_pipe_metrics_msssim_weights(self._p(), wt), "odhip_pipe_metrics_msssim_weights")
        return np.array(wt[:], np.int64).reshape(2, MSSSIM_SCALES)

    def metrics_ssim_weights(self):
        """The SSIM weight of a plane of (luma, chroma) (odhip_pipe_metrics_ssim_weights)."""
        wt = (ctypes.c_int64 * 2)()
        _check(lib().odhip_pipe_metrics_ssim_weights(self._p(), wt), "odhip_pipe_metrics_ssim_weights")
        return int(wt[0]), int(wt[1])

    def nblocks(self, set_, level):
        n = 4 << level
        dec = 1 if set_ and not self.chroma_444 else 0
        planes = self.frames * (2 if set_ else 1)
        return planes * ((self.W >> dec) // n) * ((self.H >> dec) // n)


# ---- YUV4MPEG2 input (odhip_y4m_open2) ---------------------------------------------------
Y4M_ALLOW_444, = _defines("Y4M_ALLOW_444")


class Y4M:
    """odhip_y4m_open2: progressive 8-bit 4:2:0 or (allow_444) 4:4:4 frames of a YUV4MPEG2 file.
    w, h, fps_n, fps_d and chroma_dec (1: 4:2:0, 0: 4:4:4); read() returns (luma [h][w],
    cb, cr [(h + dec) >> dec][(w + dec) >> dec]) as uint8 numpy arrays, None at the end."""

    def __init__(self, path, allow_444=True):
        L = lib()
        w, h, fn, fd, dec, err = (ctypes.c_int() for _ in range(6))
        self.h = L.odhip_y4m_open2(os.fsencode(path), Y4M_ALLOW_444 if allow_444 else 0, ctypes.byref(w),
                                   ctypes.byref(h), ctypes.byref(fn), ctypes.byref(fd), ctypes.byref(dec),
                                   ctypes.byref(err))
        if not self.h:
            raise DaalaHipError("odhip_y4m_open2(%s) failed: %d" % (path, err.value))
        self.w, self.h_px, self.fps_n, self.fps_d = w.value, h.value, fn.value, fd.value
        self.chroma_dec = dec.value
        self.cw = (self.w + self.chroma_dec) >> self.chroma_dec
        self.ch = (self.h_px + self.chroma_dec) >> self.chroma_dec

    def read(self):
        y = np.empty((self.h_px, self.w), np.uint8)
        cb = np.empty((self.ch, self.cw), np.uint8)
        cr = np.empty((self.ch, self.cw), np.uint8)
        rc = lib().odhip_y4m_read(self.h, y.ctypes.data_as(ctypes.c_void_p),
                                  cb.ctypes.data_as(ctypes.c_void_p), cr.ctypes.data_as(ctypes.c_void_p))
        if rc == 0:
            return None
        _check(rc if rc < 0 else 0, "odhip_y4m_read")
        return y, cb, cr

    def skip(self):
        """Steps over one frame: True, False at the end of the stream."""
        rc = lib().odhip_y4m_skip(self.h)
        _check(rc if rc < 0 else 0, "odhip_y4m_skip")
        return rc == 1

    def close(self):
        if self.h:
            lib().odhip_y4m_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- od_compute_dist (block-size RDO distortion) ---------------------------------------
def compute_dist(x, y, bs, use_masking=1, flat_qm=0, coded_quantizer=40):
    """od_compute_dist of every (4 << bs)-square block of x (source) against y
    (reconstruction): int32 CUDA tensors [nplanes, h, w].  The device computes everything up
    to the libm call, the host applies pow (odhip_dist_finish).  Returns (dist float64 numpy
    [nplanes, h/n, w/n], parts float64 numpy [nplanes, h/8, w/8, 3])."""
    import torch
    _need(x, torch.int32, "x")
    _need(y, torch.int32, "y")
    assert x.shape == y.shape
    nplanes, h, w = x.shape
    n = 4 << bs
    parts = torch.empty((nplanes, h // 8, w // 8, 3), dtype=torch.float64, device=x.device)
    _check(lib().odhip_dist_parts(_p(parts), _p(x), _p(y), nplanes, w, h, int(bs), int(use_masking),
                                  int(flat_qm), _stream()), "odhip_dist_parts")
    hp = parts.cpu().numpy()
    dist = np.zeros((nplanes, h // n, w // n), np.float64)
    _check(lib().odhip_dist_finish(dist.ctypes.data_as(ctypes.c_void_p),
                                   hp.ctypes.data_as(ctypes.c_void_p), nplanes, w, h, int(bs),
                                   int(use_masking), int(flat_qm), int(coded_quantizer)),
           "odhip_dist_finish")
    return dist, hp


def set_price_tol_scale(scale):
    """Test hook: multiplies the margin inside which a priced choice is left to the host
    libm (odhip_ctx_set_test_hooks on the current context and every live Pipe); 1 restores it."""
    _hooks["tol"] = float(scale)
    _apply_hooks()


# ---- quality metrics: PSNR and PSNR-HVS-M on the device (metrics_kernels.hip) ----------
METRIC_SSE, METRIC_PSNRHVS, METRIC_SSIM, METRIC_MSSSIM, METRIC_FASTSSIM, METRIC_CIEDE = _defines(
    "METRIC_SSE", "METRIC_PSNRHVS", "METRIC_SSIM", "METRIC_MSSSIM", "METRIC_FASTSSIM", "METRIC_CIEDE")
FASTSSIM_LEVELS, MSSSIM_SCALES, MSSSIM_MIN_SIZE, SSIM_MAX_RADIUS = _defines(
    "FASTSSIM_LEVELS", "MSSSIM_SCALES", "MSSSIM_MIN_SIZE", "SSIM_MAX_RADIUS")
SAMPLE_U8, SAMPLE_U16, SAMPLE_I16_12, CSF_Y, CSF_CB, CSF_CR = _defines(
    "SAMPLE_U8", "SAMPLE_U16", "SAMPLE_I16_12", "CSF_Y", "CSF_CB", "CSF_CR")
# The optional columns of a pipe's metrics slot, in the slot's order (the table of include/daala_hip.h): the keyword of
# Pipe.set_metrics - PipeMetrics has the attribute and set_<keyword> -, the flag, the trailing shape of a plane value
# (None: one entry per picture and luma level, [5][F]), and what the column's scores need besides the sums, of a Pipe
PIPE_METRIC_COLUMNS = (
    ("ssim", METRIC_SSIM, (), lambda pipe: pipe.metrics_ssim_weights()),
    ("msssim", METRIC_MSSSIM, (MSSSIM_SCALES,), lambda pipe: pipe.metrics_msssim_weights()),
    ("fastssim", METRIC_FASTSSIM, (FASTSSIM_LEVELS,), lambda pipe: ((pipe.pic_w, pipe.pic_h), (pipe.cw, pipe.ch))),
    ("ciede", METRIC_CIEDE, None, lambda pipe: (pipe.pic_w, pipe.pic_h)),
)


_MetricsPair, _CiedePair, _PipeMetricsInfo = (_S["odhip_metrics_pair"], _S["odhip_ciede_pair"],
                                              _S["odhip_pipe_metrics_info"])


def psnr_db(sse, npixels, depth=8):
    """dump_psnr's formula: 10*(log10(max^2) + log10(npixels) - log10(sse)), max = 2^depth - 1 (inf for sse 0)."""
    m = (1 << depth) - 1
    with np.errstate(divide="ignore"):
        return 10 * (np.log10(float(m * m)) + np.log10(np.asarray(npixels, np.float64))
                     - np.log10(np.asarray(sse, np.float64)))


def psnrhvs_db(hvs_sum, nwindows, depth=8):
    """dump_psnrhvs's score: 10*(-log10(sum/pixels/max^2)), pixels = 64 per window."""
    m = (1 << depth) - 1
    with np.errstate(divide="ignore"):
        return 10 * (-np.log10(np.asarray(hvs_sum, np.float64) / (64.0 * np.asarray(nwindows, np.float64))
                               / float(m * m)))


def _metric_fmt(t, fmt):
    import torch
    if fmt is not None:
        return int(fmt)
    if t.dtype == torch.uint8:
        return SAMPLE_U8
    if t.dtype == torch.int16:
        return SAMPLE_U16
    raise DaalaHipError("metrics: uint8 or int16 CUDA tensors (int16: give src_fmt / rec_fmt for 12-bit planes)")


def _metric_pairs(src, rec, w, h, depth, csf, src_fmt, rec_fmt):
    import torch
    for t in (src, rec):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 3 and t.is_contiguous()):
            raise DaalaHipError("metrics: contiguous CUDA tensors [n][rows][stride]")
    n = src.shape[0]
    assert rec.shape[0] == n
    w = src.shape[2] if w is None else int(w)
    h = src.shape[1] if h is None else int(h)
    assert w <= min(src.shape[2], rec.shape[2]) and h <= min(src.shape[1], rec.shape[1])
    csf = [int(csf)] * n if np.isscalar(csf) else [int(c) for c in csf]
    sf, rf = _metric_fmt(src, src_fmt), _metric_fmt(rec, rec_fmt)
    pairs = (_MetricsPair * max(1, n))()
    for i in range(n):
        pairs[i] = _MetricsPair(src[i].data_ptr(), rec[i].data_ptr(), sf, rf, src.shape[2], rec.shape[2], w, h,
                                int(depth), csf[i])
    return pairs, n


def metrics_planes(src, rec, w=None, h=None, depth=8, csf=CSF_Y, sse=True, psnrhvs=True, src_fmt=None,
                   rec_fmt=None):
    """odhip_metrics_planes over n plane pairs: src / rec CUDA tensors [n][rows][stride] (uint8, or int16 holding
    uint16 samples at `depth` - src_fmt / rec_fmt = SAMPLE_I16_12 for int16 planes at 12 bits), the picture region
    w x h (default: the whole plane), csf one CSF_* or one per pair.  Returns (sse int64 [n], hvs float64 [n],
    npixels [n], nwindows [n]) as numpy arrays (a metric not asked for reads 0)."""
    import torch
    pairs, n = _metric_pairs(src, rec, w, h, depth, csf, src_fmt, rec_fmt)
    d_sse = torch.zeros(max(1, n), dtype=torch.int64, device=src.device)
    d_hvs = torch.zeros(max(1, n), dtype=torch.float64, device=src.device)
    npix = (ctypes.c_long * max(1, n))()
    nwin = (ctypes.c_long * max(1, n))()
    flags = (METRIC_SSE if sse else 0) | (METRIC_PSNRHVS if psnrhvs else 0)
    _check(lib().odhip_metrics_planes(pairs, n, flags, _p(d_sse), _p(d_hvs), npix, nwin, _stream()),
           "odhip_metrics_planes")
    return (d_sse[:n].cpu().numpy(), d_hvs[:n].cpu().numpy(), np.array(npix[:n], np.int64),
            np.array(nwin[:n], np.int64))


def psnrhvs_windows(src, rec, w=None, h=None, depth=8, csf=CSF_Y, src_fmt=None, rec_fmt=None):
    """odhip_psnrhvs_windows of ONE plane pair (tensors [rows][stride]): float32 numpy [nwy][nwx], the 64 terms of
    every window summed in float in (i, j) order."""
    import torch
    pairs, _ = _metric_pairs(src[None], rec[None], w, h, depth, csf, src_fmt, rec_fmt)
    nwx, nwy = ctypes.c_int(), ctypes.c_int()
    L = lib()
    nw = L.odhip_psnrhvs_window_count(pairs[0].w, pairs[0].h, ctypes.byref(nwx), ctypes.byref(nwy))
    out = torch.zeros(max(1, nw), dtype=torch.float32, device=src.device)
    _check(L.odhip_psnrhvs_windows(ctypes.byref(pairs[0]), _p(out), _stream()), "odhip_psnrhvs_windows")
    return out[:nw].cpu().numpy().reshape(nwy.value, nwx.value)


def ssim_taps(sigma, max_len):
    """odhip_ssim_taps: the tap table of dump_ssim's gaussian_filter_init(sigma, max_len) as a list (host only)."""
    cap = 2 * max(1, int(max_len)) + 1
    buf = (ctypes.c_uint32 * cap)()
    n = lib().odhip_ssim_taps(sigma, int(max_len), buf, cap)
    if n < 0:
        _check(n, "odhip_ssim_taps")
    return list(buf[:n])


def ssim_weight(w, h, par=1.0):
    """odhip_ssim_weight: the sum of the SSIM weight moment over a w x h plane (host only)."""
    wt = ctypes.c_int64()
    _check(lib().odhip_ssim_weight(int(w), int(h), par, ctypes.byref(wt)), "odhip_ssim_weight")
    return int(wt.value)


def ssim_score(ssim_sum, weight, raw=False):
    """dump_ssim's two scores of a sum of terms and its weight (scalars or arrays): raw (-r) sum/weight, or
    10*(log10(weight) - log10(weight - sum)).  Sums and weights of several planes or frames add before the call."""
    s = np.asarray(ssim_sum, np.float64)
    wt = np.asarray(weight, np.float64)
    if raw:
        return s / wt
    with np.errstate(divide="ignore"):
        return 10 * (np.log10(wt) - np.log10(wt - s))


def ssim_planes(src, rec, w=None, h=None, depth=8, par=1.0, src_fmt=None, rec_fmt=None):
    """odhip_ssim_planes over n plane pairs (tensors as for metrics_planes): (sum of terms float64 [n], weight int64
    [n]) as numpy arrays; ssim_score turns them into the tool's scores."""
    import torch
    pairs, n = _metric_pairs(src, rec, w, h, depth, CSF_Y, src_fmt, rec_fmt)
    d_sum = torch.zeros(max(1, n), dtype=torch.float64, device=src.device)
    wt = (ctypes.c_int64 * max(1, n))()
    _check(lib().odhip_ssim_planes(pairs, n, par, _p(d_sum), wt, _stream()), "odhip_ssim_planes")
    return d_sum[:n].cpu().numpy(), np.array(wt[:n], np.int64)


def ssim_terms(src, rec, w=None, h=None, depth=8, par=1.0, src_fmt=None, rec_fmt=None):
    """odhip_ssim_terms of ONE plane pair (tensors [rows][stride]): float64 numpy [h][w], the term of every sample."""
    import torch
    pairs, _ = _metric_pairs(src[None], rec[None], w, h, depth, CSF_Y, src_fmt, rec_fmt)
    out = torch.zeros(pairs[0].w * pairs[0].h, dtype=torch.float64, device=src.device)
    _check(lib().odhip_ssim_terms(ctypes.byref(pairs[0]), par, _p(out), _stream()), "odhip_ssim_terms")
    return out.cpu().numpy().reshape(pairs[0].h, pairs[0].w)


def msssim_taps():
    """odhip_msssim_taps: the nine taps of dump_msssim's gaussian_filter_init(1.5, 5) at weight 1024, by the host libm."""
    buf = (ctypes.c_uint32 * 9)()
    _check(lib().odhip_msssim_taps(buf), "odhip_msssim_taps")
    return list(buf)


def msssim_weights(w, h):
    """odhip_msssim_weights: the sum of the weight moment over each of the five scales of a w x h plane (host only)."""
    wt = (ctypes.c_int64 * MSSSIM_SCALES)()
    _check(lib().odhip_msssim_weights(int(w), int(h), wt), "odhip_msssim_weights")
    return [int(v) for v in wt]


def msssim_score(sums, weights, raw=False):
    """dump_msssim's two scores of five sums and weights (or arrays [...][5] of them): raw (-r) the product of
    odhip_msssim_score, by the host libm's pow, or 10*(log10(1) - log10(1 - product)).  NaN where a cs is negative, as
    the tool prints."""
    s = np.ascontiguousarray(sums, np.float64)
    wt = np.ascontiguousarray(np.broadcast_to(np.asarray(weights, np.int64), s.shape))
    assert s.shape[-1] == MSSSIM_SCALES
    out = np.zeros(s.shape[:-1], np.float64)
    flat, fs, fw = out.reshape(-1), s.reshape(-1, MSSSIM_SCALES), wt.reshape(-1, MSSSIM_SCALES)
    v = ctypes.c_double()
    for i in range(flat.size):
        _check(lib().odhip_msssim_score(fs[i].ctypes.data_as(ctypes.c_void_p), fw[i].ctypes.data_as(ctypes.c_void_p),
                                        ctypes.byref(v)), "odhip_msssim_score")
        flat[i] = v.value
    if not raw:
        with np.errstate(divide="ignore", invalid="ignore"):
            out = 10 * (np.log10(1.0) - np.log10(1.0 - out))
    return float(out) if out.ndim == 0 else out


def msssim_planes(src, rec, w=None, h=None, depth=8, src_fmt=None, rec_fmt=None):
    """odhip_msssim_planes over n plane pairs (tensors as for metrics_planes, w and h at least 16): (sums float64
    [n][5] - the cs terms of scales 0..3 and the ssim terms of scale 4 - and weights int64 [n][5]) as numpy arrays;
    msssim_score turns them into the tool's scores."""
    import torch
    pairs, n = _metric_pairs(src, rec, w, h, depth, CSF_Y, src_fmt, rec_fmt)
    d_sums = torch.zeros((max(1, n), MSSSIM_SCALES), dtype=torch.float64, device=src.device)
    wt = (ctypes.c_int64 * (MSSSIM_SCALES * max(1, n)))()
    _check(lib().odhip_msssim_planes(pairs, n, _p(d_sums), wt, _stream()), "odhip_msssim_planes")
    return d_sums[:n].cpu().numpy(), np.array(wt[:MSSSIM_SCALES * n], np.int64).reshape(n, MSSSIM_SCALES)


def msssim_terms(src, rec, scale, w=None, h=None, depth=8, src_fmt=None, rec_fmt=None):
    """odhip_msssim_terms of ONE plane pair (tensors [rows][stride]) at one scale: (cs, ssim) float64 numpy
    [h >> scale][w >> scale], both terms of every sample."""
    import torch
    pairs, _ = _metric_pairs(src[None], rec[None], w, h, depth, CSF_Y, src_fmt, rec_fmt)
    ws, hs = pairs[0].w >> scale, pairs[0].h >> scale
    cs = torch.zeros(max(1, ws * hs), dtype=torch.float64, device=src.device)
    ss = torch.zeros(max(1, ws * hs), dtype=torch.float64, device=src.device)
    _check(lib().odhip_msssim_terms(ctypes.byref(pairs[0]), int(scale), _p(cs), _p(ss), _stream()), "odhip_msssim_terms")
    return cs[:ws * hs].cpu().numpy().reshape(hs, ws), ss[:ws * hs].cpu().numpy().reshape(hs, ws)


def fastssim_level_size(w, h, level):
    """odhip_fastssim_level_size: (w_l, h_l) of level 0..3 of a w x h plane (host only)."""
    wl, hl = ctypes.c_int(), ctypes.c_int()
    _check(lib().odhip_fastssim_level_size(int(w), int(h), int(level), ctypes.byref(wl), ctypes.byref(hl)),
           "odhip_fastssim_level_size")
    return wl.value, hl.value


def fastssim_tool_exact(w, h):
    """odhip_fastssim_tool_exact: True where the reference tool's downsampling reads stay inside the level they read, so
    that the library's FastSSIM is the tool's; False where the tool reads a foreign sample or row (1920 x 1080)."""
    rc = lib().odhip_fastssim_tool_exact(int(w), int(h))
    if rc < 0:
        _check(rc, "odhip_fastssim_tool_exact")
    return bool(rc)


def fastssim_score(sums, w, h, raw=False):
    """dump_fastssim's two scores of the four sums of a w x h plane (or an array [...][4] of them): raw (-r) the product
    of odhip_fastssim_score, by the host libm's pow, or 10*(log10(1) - log10(1 - product)).  NaN where a sum is
    negative, as the tool prints."""
    s = np.ascontiguousarray(sums, np.float64)
    assert s.shape[-1] == FASTSSIM_LEVELS
    out = np.zeros(s.shape[:-1], np.float64)
    flat, fs = out.reshape(-1), s.reshape(-1, FASTSSIM_LEVELS)
    v = ctypes.c_double()
    for i in range(flat.size):
        _check(lib().odhip_fastssim_score(fs[i].ctypes.data_as(ctypes.c_void_p), int(w), int(h), ctypes.byref(v)),
               "odhip_fastssim_score")
        flat[i] = v.value
    if not raw:
        with np.errstate(divide="ignore", invalid="ignore"):
            out = 10 * (np.log10(1.0) - np.log10(1.0 - out))
    return float(out) if out.ndim == 0 else out


def fastssim_planes(src, rec, w=None, h=None, depth=8, src_fmt=None, rec_fmt=None):
    """odhip_fastssim_planes over n plane pairs (tensors as for metrics_planes, w and h at least 16): the sums of the
    terms of the four levels, float64 numpy [n][4]; fastssim_score turns them into the tool's scores."""
    import torch
    pairs, n = _metric_pairs(src, rec, w, h, depth, CSF_Y, src_fmt, rec_fmt)
    d_sums = torch.zeros((max(1, n), FASTSSIM_LEVELS), dtype=torch.float64, device=src.device)
    _check(lib().odhip_fastssim_planes(pairs, n, _p(d_sums), _stream()), "odhip_fastssim_planes")
    return d_sums[:n].cpu().numpy()


def fastssim_terms(src, rec, level, w=None, h=None, depth=8, src_fmt=None, rec_fmt=None):
    """odhip_fastssim_terms of ONE plane pair (tensors [rows][stride]) at one level: float64 numpy [h_l][w_l], the term
    of every sample (at level 3 structure times luminance)."""
    import torch
    pairs, _ = _metric_pairs(src[None], rec[None], w, h, depth, CSF_Y, src_fmt, rec_fmt)
    wl, hl = fastssim_level_size(pairs[0].w, pairs[0].h, level)
    out = torch.zeros(wl * hl, dtype=torch.float64, device=src.device)
    _check(lib().odhip_fastssim_terms(ctypes.byref(pairs[0]), int(level), _p(out), _stream()), "odhip_fastssim_terms")
    return out.cpu().numpy().reshape(hl, wl)


def _ciede_pair(src, rec, w, h, depth, src_fmt, rec_fmt):
    """odhip_ciede_pair of one picture pair: src and rec are (Y, Cb, Cr) CUDA tensors [rows][stride], uint8 or int16 as
    for metrics_planes; the picture is w x h luma samples (default: the whole luma plane) and 4:2:0 where the chroma
    planes have fewer rows than h, 4:4:4 otherwise."""
    import torch
    for side in (src, rec):
        assert len(side) == 3
        for t in side:
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 and t.stride(1) == 1):
                raise DaalaHipError("ciede: (Y, Cb, Cr) CUDA tensors [rows][stride], samples of a row adjacent")
        if not (side[1].dtype == side[2].dtype == side[0].dtype and side[1].stride(0) == side[2].stride(0)):
            raise DaalaHipError("ciede: the three planes of a side share their sample type, Cb and Cr their stride")
    w = src[0].shape[1] if w is None else int(w)
    h = src[0].shape[0] if h is None else int(h)
    cdec = 1 if src[1].shape[0] < h else 0
    for side in (src, rec):
        assert side[0].shape[0] >= h and side[0].shape[1] >= w
        assert side[1].shape[0] >= h >> cdec and side[2].shape[0] >= h >> cdec
        assert min(side[1].shape[1], side[2].shape[1]) >= w >> cdec
    q = _CiedePair()
    for i in range(3):
        q.src[i] = src[i].data_ptr()
        q.rec[i] = rec[i].data_ptr()
    q.src_fmt, q.rec_fmt = _metric_fmt(src[0], src_fmt), _metric_fmt(rec[0], rec_fmt)
    q.src_stride, q.src_cstride = src[0].stride(0), src[1].stride(0)
    q.rec_stride, q.rec_cstride = rec[0].stride(0), rec[1].stride(0)
    q.w, q.h, q.depth, q.cdec = w, h, int(depth), cdec
    return q


def ciede_score(ciede_sum, w, h):
    """dump_ciede2000's score of a picture's SUM dE00 (a scalar or an array): 45 - 20*log10(sum/(w*h)) by the host
    libm (odhip_ciede_score), inf for identical pictures.  The tool's Total is the mean of the frames' scores."""
    s = np.asarray(ciede_sum, np.float64)
    out = np.zeros(s.shape, np.float64)
    flat, fs = out.reshape(-1), s.reshape(-1)
    v = ctypes.c_double()
    for i in range(flat.size):
        _check(lib().odhip_ciede_score(float(fs[i]), int(w), int(h), ctypes.byref(v)), "odhip_ciede_score")
        flat[i] = v.value
    return float(out) if out.ndim == 0 else out


def ciede_pictures(pictures, depth=8):
    """odhip_ciede_pictures over n picture pairs in ONE call: `pictures` is a list of (src, rec) or (src, rec, opts),
    src and rec each (Y, Cb, Cr) CUDA tensors [rows][stride] (uint8, or int16 holding uint16 samples at the depth -
    opts src_fmt / rec_fmt = SAMPLE_I16_12 for int16 planes at 12 bits), opts a dict of w, h, depth, src_fmt, rec_fmt.
    Chroma planes with fewer rows than h make a pair 4:2:0.  Returns SUM dE00 of every pair, float64 numpy [n];
    ciede_score turns a sum into the tool's score."""
    import torch
    n = len(pictures)
    pairs = (_CiedePair * max(1, n))()
    for i, pic in enumerate(pictures):
        o = dict(pic[2]) if len(pic) > 2 else {}
        pairs[i] = _ciede_pair(pic[0], pic[1], o.get("w"), o.get("h"), o.get("depth", depth), o.get("src_fmt"),
                               o.get("rec_fmt"))
    dev = pictures[0][0][0].device if n else "cuda"
    d_sum = torch.zeros(max(1, n), dtype=torch.float64, device=dev)
    _check(lib().odhip_ciede_pictures(pairs, n, _p(d_sum), _stream()), "odhip_ciede_pictures")
    return d_sum[:n].cpu().numpy()


def ciede_terms(src, rec, w=None, h=None, depth=8, src_fmt=None, rec_fmt=None):
    """odhip_ciede_terms of ONE picture pair (src, rec as for ciede_pictures): float64 numpy [h][w], dE00 of every
    pixel."""
    import torch
    q = _ciede_pair(src, rec, w, h, depth, src_fmt, rec_fmt)
    out = torch.zeros(q.w * q.h, dtype=torch.float64, device=src[0].device)
    _check(lib().odhip_ciede_terms(ctypes.byref(q), _p(out), _stream()), "odhip_ciede_terms")
    return out.cpu().numpy().reshape(q.h, q.w)


def ciede_lab_terms(lab1, lab2, kL=0.65, kC=1.0, kH=4.0):
    """odhip_ciede_lab_terms: dE00 of n Lab triples (arrays [n][3], source and reconstruction) with the given weights,
    through the device function k_ciede calls: float64 numpy [n]."""
    import torch
    a = torch.from_numpy(np.ascontiguousarray(lab1, np.float64).reshape(-1, 3)).cuda()
    b = torch.from_numpy(np.ascontiguousarray(lab2, np.float64).reshape(-1, 3)).cuda()
    assert a.shape == b.shape
    n = a.shape[0]
    out = torch.zeros(max(1, n), dtype=torch.float64, device=a.device)
    _check(lib().odhip_ciede_lab_terms(_p(a), _p(b), n, float(kL), float(kC), float(kH), _p(out), _stream()),
           "odhip_ciede_lab_terms")
    return out[:n].cpu().numpy()


class PipeMetrics:
    """One step's metrics taken from a Pipe: step, sse / hvs as (luma [5][F], chroma [nlev][2F]) numpy arrays (int64 /
    float64; chroma planes all Cb, then all Cr), npixels / nwindows per plane of (luma, chroma), depth, and the dB
    values of the tools' formulas: psnr() / psnrhvs() -> (luma, chroma)."""

    def __init__(self, step, sse, hvs, info, npix, nwin):
        self.step = step
        self._shapes = ((5, info.luma_planes), (info.chroma_levels, info.chroma_planes))
        self.sse, self.hvs = self._split(sse), self._split(hvs)
        self.npixels, self.nwindows, self.depth = tuple(npix), tuple(nwin), info.depth

    def _split(self, flat):
        """A column [values] or [values][k] as (luma [5][F], chroma [nlev][2F]), each [k] where the column is."""
        n = 5 * self._shapes[0][1]
        return tuple(a.reshape(s + flat.shape[1:]) for a, s in zip((flat[:n], flat[n:]), self._shapes))

    def psnr(self):
        return tuple(psnr_db(self.sse[i], self.npixels[i], self.depth) for i in (0, 1))

    def psnrhvs(self):
        return tuple(psnrhvs_db(self.hvs[i], self.nwindows[i], self.depth) for i in (0, 1))

    # the columns of PIPE_METRIC_COLUMNS: None unless set
    ssim = ssim_weights = msssim = msssim_weights = fastssim = fastssim_sizes = ciede = ciede_size = None

    def set_ssim(self, ssim, weights):
        """ssim: the sums of the terms as (luma [5][F], chroma [nlev][2F]); ssim_weights: per plane of (luma, chroma)."""
        self.ssim, self.ssim_weights = self._split(ssim), tuple(weights)

    def ssim_scores(self, raw=False):
        """The tool's score of every plane (ssim_score): (luma, chroma)."""
        return tuple(ssim_score(self.ssim[i], self.ssim_weights[i], raw) for i in (0, 1))

    def set_msssim(self, msssim, weights):
        """msssim: the five sums as (luma [5][F][5], chroma [nlev][2F][5]); msssim_weights: int64 [2][5], per plane of
        (luma, chroma)."""
        self.msssim, self.msssim_weights = self._split(msssim), np.asarray(weights, np.int64)

    def msssim_scores(self, raw=False):
        """The tool's score of every plane (msssim_score): (luma [5][F], chroma [nlev][2F])."""
        return tuple(msssim_score(self.msssim[i], self.msssim_weights[i], raw) for i in (0, 1))

    def set_fastssim(self, fastssim, sizes):
        """fastssim: the four sums as (luma [5][F][4], chroma [nlev][2F][4]); fastssim_sizes: (w, h) of a plane of
        (luma, chroma)."""
        self.fastssim, self.fastssim_sizes = self._split(fastssim), tuple(sizes)

    def fastssim_scores(self, raw=False):
        """The tool's score of every plane (fastssim_score): (luma [5][F], chroma [nlev][2F])."""
        return tuple(fastssim_score(self.fastssim[i], *self.fastssim_sizes[i], raw=raw) for i in (0, 1))

    def set_ciede(self, ciede, size):
        """ciede: SUM dE00 of every picture at every luma level, [5][F]; ciede_size: (w, h) of a picture."""
        self.ciede, self.ciede_size = ciede.reshape(5, -1), tuple(size)

    def ciede_scores(self):
        """The tool's score of every picture and luma level (ciede_score): [5][F]."""
        return ciede_score(self.ciede, *self.ciede_size)


# ---- motion compensation from motion-vector grids (mc_kernels.hip) ----
# odhip_mv_point and its numpy layout; grids are [pictures][coded_h/8 + 1][coded_w/8 + 1]
_MvPoint, _McJob = _S["odhip_mv_point"], _S["odhip_mc_job"]
MV_POINT = np.dtype(_MvPoint)


class MotionRangeError(DaalaHipError):
    """A grid's vector takes a filter window outside the border the reference replicates round its frames
    (ODHIP_ERANGE): nothing was launched."""


def _mc_grid(grid, coded_w, coded_h):
    g = np.ascontiguousarray(grid, MV_POINT)
    if g.ndim == 2:
        g = g[None]
    if g.ndim != 3 or g.shape[1:] != (coded_h // 8 + 1, coded_w // 8 + 1):
        raise DaalaHipError("mc: grid [pictures][coded_h/8 + 1][coded_w/8 + 1] of MV_POINT")
    return g


def mc_check_grid(grid, coded_w, coded_h, dec=0, nrefs=1):
    """odhip_mc_check_grid of a host grid: 0, or the ODHIP_* code (ERANGE: a vector outside the legal range)."""
    g = _mc_grid(grid, coded_w, coded_h)
    return lib().odhip_mc_check_grid(g.ctypes.data_as(ctypes.c_void_p), int(coded_w), int(coded_h), g.shape[0],
                                     int(dec), int(nrefs))


def mc_predict(refs, grid, dec=0, out=None):
    """odhip_mc_predict_planes: refs = 1..3 CUDA tensors [nplanes][coded_h >> dec][coded_w >> dec], one per reference
    slot (uint8, or int16 at 12 bits), grid = MV_POINT array [F][coded_h/8 + 1][coded_w/8 + 1] (numpy: checked,
    MotionRangeError outside the legal range) or a CUDA uint8 tensor holding the same bytes (the caller has checked
    it); nplanes a multiple of F, plane p predicted from grid p % F.  Returns the prediction, shaped like refs[0]."""
    import torch
    refs = list(refs)
    r0 = refs[0]
    for t in refs:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 3 and t.is_contiguous()
                and t.dtype == r0.dtype and t.shape == r0.shape):
            raise DaalaHipError("mc_predict: contiguous CUDA tensors [nplanes][rows][cols] of one shape and type")
    if r0.dtype not in (torch.uint8, torch.int16) or not 1 <= len(refs) <= 3:
        raise DaalaHipError("mc_predict: 1..3 uint8 or int16 reference plane sets")
    nplanes, h, w = r0.shape
    coded_w, coded_h = w << dec, h << dec
    on_device = isinstance(grid, torch.Tensor)
    if on_device:
        _need(grid, torch.uint8, "grid")
        per = MV_POINT.itemsize * (coded_h // 8 + 1) * (coded_w // 8 + 1)
        npics = grid.numel() // per
        if grid.numel() != npics * per or not grid.is_contiguous():
            raise DaalaHipError("mc_predict: a device grid holds whole [coded_h/8 + 1][coded_w/8 + 1] grids of MV_POINT")
        gptr = grid.data_ptr()
    else:
        g = _mc_grid(grid, coded_w, coded_h)
        npics = g.shape[0]
        gptr = g.ctypes.data
    if npics < 1 or nplanes % npics:
        raise DaalaHipError("mc_predict: the planes of a set are a multiple of the grids")
    if out is None:
        out = torch.empty_like(r0)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == r0.device and out.is_contiguous()
              and out.dtype == r0.dtype and out.shape == r0.shape):
        raise DaalaHipError("mc_predict: out is a contiguous CUDA tensor shaped and typed like refs[0]")
    job = _McJob(coded_w=coded_w, coded_h=coded_h, dec=int(dec),
                 sample=SAMPLE_U8 if r0.dtype == torch.uint8 else SAMPLE_I16_12, npics=npics, nplanes=nplanes,
                 nrefs=len(refs), grid_on_device=int(on_device), ref_stride=w, dst_stride=out.shape[2],
                 ref_plane_stride=h * w, dst_plane_stride=out.shape[1] * out.shape[2],
                 ref=(ctypes.c_void_p * 3)(*[t.data_ptr() for t in refs]), dst=out.data_ptr(), grid=gptr)
    rc = lib().odhip_mc_predict_planes(ctypes.byref(job), _stream())
    if rc == ERANGE:
        raise MotionRangeError("odhip_mc_predict_planes: a vector is outside the legal range")
    _check(rc, "odhip_mc_predict_planes")
    return out


def mc_leaves(grid, coded_w, coded_h):
    """odhip_mc_leaves: per picture the sorted uint32 leaf descriptors the device walk finds
    (vx | vy << 12 | log2(size/8) << 24 | outside corner << 26 | split flags << 28)."""
    g = _mc_grid(grid, coded_w, coded_h)
    cap = (coded_w // 8) * (coded_h // 8)
    out = np.zeros((g.shape[0], cap), np.uint32)
    counts = (ctypes.c_int * g.shape[0])()
    _check(lib().odhip_mc_leaves(g.ctypes.data_as(ctypes.c_void_p), int(coded_w), int(coded_h), g.shape[0],
                                 out.ctypes.data_as(ctypes.c_void_p), counts, cap), "odhip_mc_leaves")
    return [out[i, :counts[i]].copy() for i in range(g.shape[0])]


# ---- motion search: grids by exhaustive block matching (me_kernels.hip) ----
ME_CAND = np.dtype(_S["odhip_me_cand"])
# odhip_me_job .. odhip_me_job4, each holding the one before as its first field; `lambda` is spelled lambda_
MeJob, MeJob2, MeJob3, MeJob4 = _S["odhip_me_job"], _S["odhip_me_job2"], _S["odhip_me_job3"], _S["odhip_me_job4"]
ME_CHROMA, ME_SATD = _defines("ME_CHROMA", "ME_SATD")


def _me_job(src, refs, pic_w, pic_h, log_size, rng, res, lam):
    """src: uint8 CUDA [F][rows >= pic_h][cols >= pic_w] (any strides with unit column stride), refs: 1..3 uint8 CUDA
    [F][coded_h][coded_w] of one shape and one set of strides."""
    import torch
    refs = list(refs)
    for t in [src] + refs:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3
                and t.stride(2) == 1):
            raise DaalaHipError("me: uint8 CUDA tensors [pictures][rows][cols] with unit column stride")
    def plane_stride(t):
        # (the stride of a dimension of one element is arbitrary)
        return t.stride(0) if t.shape[0] > 1 else t.stride(1)*t.shape[1]

    r0 = refs[0]
    if not 1 <= len(refs) <= 3 or src.shape[0] != r0.shape[0] or any(
            t.shape != r0.shape or t.stride(1) != r0.stride(1) or plane_stride(t) != plane_stride(r0) for t in refs):
        raise DaalaHipError("me: 1..3 reference plane sets of one shape and layout, one plane per picture")
    ptrs = [t.data_ptr() for t in refs] + [0]*(3 - len(refs))
    return MeJob(r0.shape[2], r0.shape[1], int(pic_w), int(pic_h), src.shape[0], len(refs), int(log_size), int(rng),
                 int(res), int(lam), src.stride(1), r0.stride(1), plane_stride(src), plane_stride(r0), src.data_ptr(),
                 (ctypes.c_void_p * 3)(*ptrs), None, None)


def _me_run_search(job, luma, fn, name, want_cost, device):
    """Gives the job's luma half its grid and cost buffers, runs fn(job), reads (grid, cost) back as numpy arrays."""
    import torch
    shape = (luma.npics, luma.coded_h // 8 + 1, luma.coded_w // 8 + 1)
    grid = torch.empty(shape + (MV_POINT.itemsize,), dtype=torch.uint8, device=device)
    cost = torch.empty(shape, dtype=torch.int32, device=device) if want_cost else None
    luma.grid = grid.data_ptr()
    luma.cost = cost.data_ptr() if want_cost else None
    _check(fn(ctypes.byref(job), _stream()), name)
    g = grid.cpu().numpy().view(MV_POINT).reshape(shape)
    return g, (cost.cpu().numpy().view(np.uint32) if want_cost else None)


def _me_cands(cands, device):
    """(the ME_CAND array flattened, its copy on the device)."""
    import torch
    c = np.ascontiguousarray(cands, ME_CAND).ravel()
    return c, torch.from_numpy(c.view(np.uint8)).to(device)


def me_search(src, refs, pic_w, pic_h, log_size, rng, res=0, lam=0, want_cost=True):
    """odhip_me_search: (grid, cost) as numpy arrays - MV_POINT [F][coded_h/8 + 1][coded_w/8 + 1] and uint32 of the
    same shape (None without want_cost).  Syncs the current stream to read them back."""
    job = _me_job(src, refs, pic_w, pic_h, log_size, rng, res, lam)
    return _me_run_search(job, job, lib().odhip_me_search, "odhip_me_search", want_cost, src.device)


def me_limits(coded_w, coded_h, log_size, vx, vy):
    """odhip_me_limits: the legal full-pel (xmin, xmax, ymin, ymax) of a valid point."""
    lim = (ctypes.c_int * 4)()
    _check(lib().odhip_me_limits(int(coded_w), int(coded_h), int(log_size), int(vx), int(vy), lim), "odhip_me_limits")
    return tuple(lim)


def me_costs(src, refs, pic_w, pic_h, log_size, cands):
    """odhip_me_costs: the SAD of every listed candidate (ME_CAND array), as uint32."""
    import torch
    job = _me_job(src, refs, pic_w, pic_h, log_size, 0, 0, 0)
    c, d_c = _me_cands(cands, src.device)
    d_sad = torch.empty(max(c.size, 1), dtype=torch.int32, device=src.device)
    _check(lib().odhip_me_costs(ctypes.byref(job), _p(d_c), c.size, _p(d_sad), _stream()), "odhip_me_costs")
    return d_sad.cpu().numpy().view(np.uint32)[:c.size]


# ---- the search with chroma in the cost and SATD as the sub-pel metric (odhip_me_search2) ----
def _me_job2(src, refs, pic_w, pic_h, log_size, rng, res, lam, lam_subpel, flags, csrc, crefs, cdec):
    """_me_job plus the chroma half: csrc uint8 CUDA [2F][rows][cols] (all Cb, then all Cr), crefs one
    [2F][coded_h >> cdec][coded_w >> cdec] per slot; both may be None without ME_CHROMA."""
    job = MeJob2(luma=_me_job(src, refs, pic_w, pic_h, log_size, rng, res, lam))
    job.flags, job.cdec, job.lambda_subpel = int(flags), int(cdec), int(lam if lam_subpel is None else lam_subpel)
    if csrc is not None:
        crefs = list(crefs)
        c0 = crefs[0]
        if len(crefs) != len(list(refs)) or any(t.dim() != 3 or t.stride(2) != 1 or t.shape[0] != 2*src.shape[0]
                                                 for t in [csrc] + crefs) or any(
                t.shape != c0.shape or t.stride() != c0.stride() for t in crefs):
            raise DaalaHipError("me: chroma as [2F][rows][cols] uint8 CUDA tensors, one reference set per slot")
        job.csrc_stride, job.cref_stride = csrc.stride(1), c0.stride(1)
        job.csrc_plane_stride, job.cref_plane_stride = csrc.stride(0), c0.stride(0)
        job.csrc = csrc.data_ptr()
        job.cref = (ctypes.c_void_p * 3)(*([t.data_ptr() for t in crefs] + [0]*(3 - len(crefs))))
    return job


def me_search2(src, refs, pic_w, pic_h, log_size, rng, res=0, lam=0, lam_subpel=None, flags=0, csrc=None, crefs=None,
               cdec=1, want_cost=True):
    """odhip_me_search2: (grid, cost) as me_search gives them; the cost is stage 2's."""
    job = _me_job2(src, refs, pic_w, pic_h, log_size, rng, res, lam, lam_subpel, flags, csrc, crefs, cdec)
    return _me_run_search(job, job.luma, lib().odhip_me_search2, "odhip_me_search2", want_cost, src.device)


def me_costs2(src, refs, pic_w, pic_h, log_size, cands, metric, flags=0, csrc=None, crefs=None, cdec=1):
    """odhip_me_costs2: uint32 [n][3], the unshifted Y, Cb, Cr distortions of every listed candidate under metric
    0 (SAD) / 1 (SATD); chroma 0 without ME_CHROMA."""
    import torch
    job = _me_job2(src, refs, pic_w, pic_h, log_size, 0, 0, 0, 0, flags, csrc, crefs, cdec)
    c, d_c = _me_cands(cands, src.device)
    d_out = torch.empty((max(c.size, 1), 3), dtype=torch.int32, device=src.device)
    _check(lib().odhip_me_costs2(ctypes.byref(job), _p(d_c), c.size, int(metric), _p(d_out),
                                 _stream()), "odhip_me_costs2")
    return d_out.cpu().numpy().view(np.uint32)[:c.size]


# ---- the search coarse to fine (odhip_me_search3) ----
def _me_job3(src, refs, pic_w, pic_h, log_size, rng, res, lam, lam_subpel, flags, csrc, crefs, cdec, levels, refine):
    """(_me_job2 plus levels and refine, the scratch tensor the job points into - keep it alive - or None)."""
    import torch
    job = MeJob3(base=_me_job2(src, refs, pic_w, pic_h, log_size, rng, res, lam, lam_subpel, flags, csrc, crefs, cdec),
                 levels=int(levels), refine=int(refine))
    need = lib().odhip_me_scratch_bytes(ctypes.byref(job))
    scratch = torch.empty(need, dtype=torch.uint8, device=src.device) if need else None
    if need:
        job.scratch, job.scratch_bytes = scratch.data_ptr(), need
    return job, scratch


def me_search3(src, refs, pic_w, pic_h, log_size, rng, res=0, lam=0, lam_subpel=None, flags=0, csrc=None, crefs=None,
               cdec=1, levels=0, refine=2, want_cost=True):
    """odhip_me_search3: me_search2 coarse to fine over `levels` halvings; (grid, cost) as me_search gives them."""
    job, scratch = _me_job3(src, refs, pic_w, pic_h, log_size, rng, res, lam, lam_subpel, flags, csrc, crefs, cdec,
                            levels, refine)
    out = _me_run_search(job, job.base.luma, lib().odhip_me_search3, "odhip_me_search3", want_cost, src.device)
    del scratch                       # (read back above: the search is done)
    return out


# ---- the search at variable block sizes (odhip_me_search_vbs) ----
def _me_job4(src, refs, pic_w, pic_h, log_min, log_max, rng, res, lam, lam_subpel, flags, csrc, crefs, cdec, levels,
             refine, split_penalty):
    """(_me_job3 at log_max plus log_min and the penalty, the scratch tensor of the whole call - keep it alive - or
    None)."""
    import torch
    base, _ = _me_job3(src, refs, pic_w, pic_h, log_max, rng, res, lam, lam_subpel, flags, csrc, crefs, cdec, levels,
                       refine)
    job = MeJob4(base=base, log_min=int(log_min), split_penalty=int(split_penalty))
    need = lib().odhip_me_vbs_scratch_bytes(ctypes.byref(job))
    scratch = torch.empty(need, dtype=torch.uint8, device=src.device) if need else None
    job.base.scratch, job.base.scratch_bytes = (scratch.data_ptr(), need) if need else (None, 0)
    return job, scratch


def me_search_vbs(src, refs, pic_w, pic_h, log_min, log_max, rng, res=0, lam=0, lam_subpel=None, flags=0, csrc=None,
                  crefs=None, cdec=1, levels=0, refine=2, split_penalty=0, want_cost=True, want_cell_dist=False):
    """odhip_me_search_vbs: a grid of leaves of 8 << log_min .. 8 << log_max pixels.  (grid, cost) as me_search gives
    them, and with want_cell_dist the 8x8 cells' distortions under every size's prediction as a third value, uint32
    [log_max - log_min + 1][F][coded_h/8][coded_w/8] (None when log_min == log_max: nothing is decided)."""
    import torch
    job, scratch = _me_job4(src, refs, pic_w, pic_h, log_min, log_max, rng, res, lam, lam_subpel, flags, csrc, crefs,
                            cdec, levels, refine, split_penalty)
    luma = job.base.base.luma
    dist = None
    if want_cell_dist and log_min != log_max:
        dist = torch.empty((log_max - log_min + 1, luma.npics, luma.coded_h // 8, luma.coded_w // 8), dtype=torch.int32,
                           device=src.device)
        job.cell_dist = dist.data_ptr()
    out = _me_run_search(job, luma, lib().odhip_me_search_vbs, "odhip_me_search_vbs", want_cost, src.device)
    del scratch                       # (read back above: the search is done)
    if want_cell_dist:
        out = out + (dist.cpu().numpy().view(np.uint32) if dist is not None else None,)
    return out


def me_cell_dist(src, refs, pic_w, pic_h, preds):
    """odhip_me_cell_dist: the SAD of every prediction in preds (1..4 contiguous uint8 CUDA tensors shaped like
    refs[0]) against src over every 8x8 cell, clipped to the picture: uint32 [len(preds)][F][coded_h/8][coded_w/8]."""
    import torch
    job = _me_job(src, refs, pic_w, pic_h, 0, 0, 0, 0)
    preds = list(preds)
    if any(not t.is_contiguous() or t.shape != refs[0].shape or t.dtype != torch.uint8 for t in preds):
        raise DaalaHipError("me_cell_dist: contiguous uint8 predictions shaped like the reference planes")
    ptrs = (ctypes.c_void_p * len(preds))(*[t.data_ptr() for t in preds])
    dist = torch.empty((len(preds), job.npics, job.coded_h // 8, job.coded_w // 8), dtype=torch.int32,
                       device=src.device)
    _check(lib().odhip_me_cell_dist(ctypes.byref(job), ptrs, len(preds), _p(dist), _stream()), "odhip_me_cell_dist")
    return dist.cpu().numpy().view(np.uint32)


def me_costs3(src, refs, pic_w, pic_h, log_size, cands, level, levels):
    """odhip_me_costs3: uint32 [n], the luma SAD of every listed candidate on pyramid level `level` of a job of
    `levels` halvings."""
    import torch
    job, scratch = _me_job3(src, refs, pic_w, pic_h, log_size, 0, 0, 0, 0, 0, None, None, 0, levels, 1)
    c, d_c = _me_cands(cands, src.device)
    d_sad = torch.empty(max(c.size, 1), dtype=torch.int32, device=src.device)
    _check(lib().odhip_me_costs3(ctypes.byref(job), _p(d_c), c.size, int(level), _p(d_sad), _stream()),
           "odhip_me_costs3")
    out = d_sad.cpu().numpy().view(np.uint32)[:c.size]
    del scratch
    return out


def me_downsample(src):
    """odhip_me_downsample: one halving of uint8 CUDA planes [n][h][w] (any strides with unit column stride), as a new
    contiguous tensor [n][(h + 1) >> 1][(w + 1) >> 1]."""
    import torch
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8 and src.dim() == 3
            and src.stride(2) == 1):
        raise DaalaHipError("me: uint8 CUDA planes [n][rows][cols] with unit column stride")
    n, h, w = src.shape
    dst = torch.empty((n, (h + 1) >> 1, (w + 1) >> 1), dtype=torch.uint8, device=src.device)
    ps = src.stride(0) if n > 1 else src.stride(1)*h
    _check(lib().odhip_me_downsample(_p(dst), dst.stride(1), dst.stride(0), _p(src), src.stride(1),
                                     ps, w, h, n, _stream()), "odhip_me_downsample")
    return dst


# ---- lossless and Haar-wavelet frames (haar_kernels.hip) ------------------------------------------------------------
HaarJob = _S["odhip_haar_job"]


def haar_planes(x, ln, inverse=False, out=None):
    """od_haar (od_haar_inv with `inverse`) of every (1 << ln)-square block of int32 CUDA planes [nplanes, h, w],
    ln = 2..6 (odhip_haar_planes)."""
    import torch
    _need(x, torch.int32, "x")
    nplanes, h, w = x.shape
    if out is None:
        out = torch.empty_like(x)
    _need(out, torch.int32, "out")
    _check(lib().odhip_haar_planes(_p(out), _p(x), nplanes, w, h, int(ln), int(bool(inverse)), _stream()),
           "odhip_haar_planes")
    return out


def _haar_job(shape, dec, pic_w, pic_h, depth, quant, dc_quant, plane_split):
    nplanes, h, w = shape
    dcq = (int(dc_quant),) * 2 if np.isscalar(dc_quant) else tuple(int(v) for v in dc_quant)
    job = HaarJob()
    job.px_plane_stride, job.px_stride, job.nplanes, job.w, job.h, job.dec = h * w, w, nplanes, w, h, int(dec)
    job.pic_w, job.pic_h = int(w if pic_w is None else pic_w), int(h if pic_h is None else pic_h)
    job.lossless, job.depth, job.quant = int(quant == 0), int(depth), int(quant)
    job.dc_quant = (ctypes.c_int32 * 2)(*dcq)
    job.plane_split = int(nplanes if plane_split is None else plane_split)
    return job


def _haar_opt(t, like, dtype, what):
    if t is not None:
        _need(t, dtype, what)
        if t.shape != like:
            raise DaalaHipError("%s must be %s" % (what, tuple(like)))
        return t.data_ptr()
    return None


def haar_encode(px, pred=None, dec=0, pic_w=None, pic_h=None, depth=8, quant=0, dc_quant=1, plane_split=None,
                want_rec=True, dc_rec=None):
    """odhip_haar_encode_planes: the coded Haar-wavelet path of the planes px (uint8, int16 in a
    full-precision-references context; [nplanes, h, w] CUDA), a keyframe's or, with the prediction planes `pred`, an
    inter frame's.  quant = state.quantizer, 0 = lossless; dc_quant one value or (below plane_split, the rest).
    Returns (q, tree, rec): int32 [nplanes, h, w] quantised coefficients with the coded DC symbol in each block's DC
    slot, the tree sums, the reconstructed samples (None without want_rec).  dc_rec: an int32 tensor
    [nplanes, superblocks] that receives the reconstructed superblock DCs."""
    import torch
    dt = px_dtype()
    _need(px, dt, "px")
    nplanes, h, w = px.shape
    job = _haar_job(px.shape, dec, pic_w, pic_h, depth, quant, dc_quant, plane_split)
    q = torch.empty((nplanes, h, w), dtype=torch.int32, device=px.device)
    tree = torch.empty_like(q)
    rec = torch.empty_like(px) if want_rec else None
    tile = 64 >> int(dec)
    job.d_px, job.d_pred = px.data_ptr(), _haar_opt(pred, px.shape, dt, "pred")
    job.d_q, job.d_tree, job.d_rec = q.data_ptr(), tree.data_ptr(), rec.data_ptr() if want_rec else None
    job.d_dc_rec = _haar_opt(dc_rec, (nplanes, (h // tile) * (w // tile)), torch.int32, "dc_rec")
    _check(lib().odhip_haar_encode_planes(ctypes.byref(job), _stream()), "odhip_haar_encode_planes")
    return q, tree, rec


def haar_decode(q, pred=None, dec=0, depth=8, quant=0, dc_quant=1, plane_split=None, dc_rec=None):
    """odhip_haar_decode_planes: the decoder's half, from the symbols q (what haar_encode returns first, not written)
    and the optional prediction to the reconstructed samples, through the kernels the encoder runs behind its
    quantiser."""
    import torch
    dt = px_dtype()
    _need(q, torch.int32, "q")
    nplanes, h, w = q.shape
    job = _haar_job(q.shape, dec, None, None, depth, quant, dc_quant, plane_split)
    rec = torch.empty((nplanes, h, w), dtype=dt, device=q.device)
    tile = 64 >> int(dec)
    job.d_pred, job.d_q, job.d_rec = _haar_opt(pred, q.shape, dt, "pred"), q.data_ptr(), rec.data_ptr()
    job.d_dc_rec = _haar_opt(dc_rec, (nplanes, (h // tile) * (w // tile)), torch.int32, "dc_rec")
    _check(lib().odhip_haar_decode_planes(ctypes.byref(job), _stream()), "odhip_haar_decode_planes")
    return rec


# ---- a frame's block-size map by activity masking (bsize_kernels.hip) -------------------
BSIZE_TERMS, = _defines("BSIZE_TERMS")


def bsize_set_test_hooks(margin_scale=1.0, perturb=False):
    """Test hooks of the block-size decision on the calling thread's current context
    (odhip_ctx_set_bsize_test_hooks): a factor on the libm margin, and a deliberately wrong device result for
    every listed cell.  The defaults restore normal operation."""
    _check(lib().odhip_ctx_set_bsize_test_hooks(None, float(margin_scale), int(bool(perturb))),
           "odhip_ctx_set_bsize_test_hooks")


def _bsize_quant(quantizer, nframes):
    q = np.ascontiguousarray(np.broadcast_to(np.asarray(quantizer, dtype=np.int32), (nframes,)))
    return q


def _bsize_args(px, quantizer, pred, out, w, h):
    """The argument list odhip_bsize_decide, _resolve and _terms share.  px (and pred): uint8 CUDA
    [frames, rows, stride] or [rows, stride]; w, h (default: the whole tensor) select the top-left w x h of
    every frame.  out: a uint8 CUDA map [frames, >= h/8, >= w/8] to write into (its top-left corner)."""
    import torch
    _need(px, torch.uint8, "px")
    single = px.dim() == 2
    px3 = px[None] if single else px
    nframes, rows, stride = px3.shape
    w = stride if w is None else int(w)
    h = rows if h is None else int(h)
    if w > stride or h > rows:
        raise DaalaHipError("w, h exceed the px tensor")
    args_pred = (None, 0, 0)
    if pred is not None:
        _need(pred, torch.uint8, "pred")
        pred3 = pred[None] if pred.dim() == 2 else pred
        if pred3.shape[0] != nframes or pred3.shape[1] < h or pred3.shape[2] < w:
            raise DaalaHipError("pred must hold %d frames of at least %d x %d" % (nframes, h, w))
        args_pred = (_p(pred3), pred3.shape[2], pred3.shape[1] * pred3.shape[2])
    if out is None:
        out = torch.empty((nframes, max(h // 8, 0), max(w // 8, 0)), dtype=torch.uint8, device=px.device)
    _need(out, torch.uint8, "out")
    if out.dim() != 3 or out.shape[0] != nframes or out.shape[1] < h // 8 or out.shape[2] < w // 8:
        raise DaalaHipError("out must be uint8 [%d, >= %d, >= %d]" % (nframes, h // 8, w // 8))
    q = _bsize_quant(quantizer, nframes)
    args = (_p(out), out.shape[2], out.shape[1] * out.shape[2], _p(px3), stride, rows * stride) + args_pred + (
        nframes, w, h, _np_p(q), _stream())
    return args, q, out, single, (nframes, h // 32, w // 32)


def bsize_decide(px, quantizer, pred=None, out=None, w=None, h=None, resolve=True):
    """odhip_bsize_decide + odhip_bsize_resolve: the block-size map of every frame by the reference's activity
    masking (od_split_superblock per 32x32 cell).  px: uint8 CUDA [frames, h, w] (or [h, w]); quantizer: one int
    (od_state.quantizer scaled by 1 << OD_COEFF_SHIFT) or one per frame; pred: the prediction, same shape, or
    None for keyframes.  Returns (bmap, relisted): bmap uint8 CUDA [frames, h/8, w/8] ([h/8, w/8] for a 2-D px),
    accepted as it is by forward_partition, inverse_partition and partition_leaves at dec = 0; relisted: the
    cells decided again on the host (None with resolve=False: asynchronous, the map's listed cells are then the
    device's).  out, w, h: see _bsize_args (strided buffers)."""
    args, q, bmap, single, _ = _bsize_args(px, quantizer, pred, out, w, h)
    _check(lib().odhip_bsize_decide(*args), "odhip_bsize_decide")
    n = None
    if resolve:
        c = ctypes.c_int(0)
        _check(lib().odhip_bsize_resolve(*(args + (ctypes.byref(c),))), "odhip_bsize_resolve")
        n = c.value
    return (bmap[0] if single and out is None else bmap), n


def bsize_terms(px, quantizer, pred=None, out=None, w=None, h=None):
    """odhip_bsize_terms: (bmap, noise, psy, relisted) - the map as from bsize_decide and, per cell, the 90 noise
    averages (numpy int32 [frames, h/32, w/32, 90]) and the 90 psy values (float32, same shape) it was decided
    from, in the order include/daala_hip.h gives."""
    import torch
    args, q, bmap, single, cells = _bsize_args(px, quantizer, pred, out, w, h)
    noise = torch.zeros(cells + (BSIZE_TERMS,), dtype=torch.int32, device=px.device)
    psy = torch.zeros(cells + (BSIZE_TERMS,), dtype=torch.float32, device=px.device)
    c = ctypes.c_int(0)
    _check(lib().odhip_bsize_terms(*((_p(noise), _p(psy)) + args + (ctypes.byref(c),))), "odhip_bsize_terms")
    return (bmap[0] if single and out is None else bmap), noise.cpu().numpy(), psy.cpu().numpy(), c.value


def bsize_terms_host(px, quantizer, pred=None, margin_scale=1.0):
    """odhip_bsize_terms_host: one plane on numpy arrays (uint8 [h, w]; a view with wider rows is passed with its
    stride), no GPU: (bmap uint8 [h/8, w/8], noise int32 [h/32, w/32, 90], psy float32 [h/32, w/32, 90], listed -
    the cells a device run would list at margin_scale times the margin, judged from libm's terms)."""
    px = np.asarray(px)
    if px.dtype != np.uint8 or px.ndim != 2 or px.strides[1] != 1:
        raise DaalaHipError("px must be uint8 [h, w] with contiguous rows")
    h, w = px.shape
    ppred, spred = None, 0
    if pred is not None:
        pred = np.asarray(pred)
        if pred.dtype != np.uint8 or pred.shape != px.shape or pred.strides[1] != 1:
            raise DaalaHipError("pred must be uint8 [h, w] like px")
        ppred, spred = _np_p(pred), pred.strides[0]
    bmap = np.zeros((max(h // 8, 0), max(w // 8, 0)), np.uint8)
    noise = np.zeros((max(h // 32, 0), max(w // 32, 0), BSIZE_TERMS), np.int32)
    psy = np.zeros(noise.shape, np.float32)
    listed = ctypes.c_int(0)
    _check(lib().odhip_bsize_terms_host(_np_p(noise), _np_p(psy), _np_p(bmap), bmap.shape[1], _np_p(px),
                                        px.strides[0], ppred, spred, w, h, int(quantizer), float(margin_scale),
                                        ctypes.byref(listed)), "odhip_bsize_terms_host")
    return bmap, noise, psy, listed.value


def bsize_decide_host(px, quantizer, pred=None):
    """odhip_bsize_decide_host: the map alone, uint8 [h/8, w/8]; numpy in, numpy out, no GPU."""
    px = np.ascontiguousarray(px, dtype=np.uint8)
    h, w = px.shape
    if pred is not None:
        pred = np.ascontiguousarray(pred, dtype=np.uint8)
    bmap = np.zeros((max(h // 8, 0), max(w // 8, 0)), np.uint8)
    _check(lib().odhip_bsize_decide_host(_np_p(bmap), bmap.shape[1], _np_p(px), w, None if pred is None else _np_p(pred),
                                         w, w, h, int(quantizer)), "odhip_bsize_decide_host")
    return bmap
