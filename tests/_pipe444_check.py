"""Whole-frame checker of the 4:4:4 frame-batch step (odhip_pipe with chroma_444 = 1) - TEST
INFRASTRUCTURE for tests/test_gpu_pipe444.py, modelled on tests/_pipeline_check.py.

cpu_frame444()  one 4:4:4 picture through the REFERENCE's own C functions (oracle/_ref:
                ref_stage_plane_levels at dec 0 for all three planes, five levels each, with
                the dec-0 QM slices).  Keyframe chroma takes as its chroma-from-luma reference
                at level bs the dequantised luma plane of the SAME level - the copy branch of
                od_resample_luma_coeffs (src/intra.c:95-108), which at 4:4:4 copies the whole
                decoded luma block.
gpu_pipe444()   an odhip_pipe with chroma_444 = 1, loaded with F pictures.
recon444() / decisions444() read what the pipe's last step left, in the shapes the
                comparisons below take."""
import ctypes
import time

import numpy as np

from _libs import P, oracle, ref

NBANDS = [1, 4, 7, 9, 9]


def pictures444(content, index, seed, pw, ph):
    """[Y, Cb, Cr] uint8 pictures of pw x ph, all three full size.  'checker': bench.py's synthetic
    frame, its chroma planes upsampled (edges and texture of their own); 'natural': the AR(1) +
    cosine content, chroma a gain of luma plus independent noise (what chroma from luma is for)."""
    import bench
    rng = np.random.RandomState(seed + 31 * index)
    if content == "checker":
        fr = bench.synth_frame_np(index, seed)
        y = fr[0][:ph, :pw]
        c = [np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:ph, :pw] for p in fr[1:]]
        c = [np.clip(p.astype(np.int32) + rng.randint(-4, 5, size=p.shape), 0, 255).astype(np.uint8) for p in c]
    else:
        fr = bench.natural_like_frame_np(index, seed)
        y = fr[0][:ph, :pw]
        d = y.astype(np.int32) - 128
        c = [np.clip(128 + g * d / 10 + rng.randint(-3, 4, size=d.shape), 0, 255).astype(np.uint8)
             for g in (6, -4)]
    return [np.ascontiguousarray(y)] + [np.ascontiguousarray(p) for p in c]


def _tables(qt, pli):
    """dec-0 QM slices for every plane; per-band steps per plane (pvq_qm_q4[pli])."""
    qm_off = (ctypes.c_int * 5)(*[int(qt.qm_offset[bs][0]) for bs in range(5)])
    qb = (ctypes.c_int * 60)()
    bb = (ctypes.c_int * 60)()
    for bs in range(5):
        for i, v in enumerate(qt.q_band(pli, bs)):
            qb[bs * 12 + i] = v
        for i, v in enumerate(qt.beta_band(pli, bs)):
            bb[bs * 12 + i] = v
    return qm_off, qb, bb


def _pad(px, pic, fpr_bits):
    h, w = px.shape
    if fpr_bits:
        oracle().odo_img_plane_copy_pad16(P(px), w, w, h, P(pic), fpr_bits, pic.shape[1], pic.shape[1],
                                          pic.shape[0])
    else:
        oracle().odo_img_plane_copy_pad(P(px), w, w, h, P(pic), pic.shape[1], pic.shape[1], pic.shape[0])


def cpu_frame444(qt, pics, pic_w, pic_h, chroma_cfl=True, lam=0.147, fpr_bits=0, inter_pred=None, decisions=None):
    """pics: [Y, Cb, Cr] pictures of pic_w x pic_h.  Returns (recon, blocks): recon[pli][bs] = the
    plane of the coded size reconstructed at uniform level bs (uint16 with fpr_bits).  decisions:
    a list that receives, per plane, [(y int32 [blocks][len], band int32 [blocks][nb][4])] per
    level (ref_stage_set_dump)."""
    r = ref()
    assert r is not None, "oracle/_ref/libdaalaref.so not built"
    r.ref_stage_plane_levels.restype = ctypes.c_long
    r.ref_set_fpr(1 if fpr_bits else 0)
    r.ref_stage_set_inter(1 if inter_pred is not None else 0)
    try:
        pdt = np.uint16 if fpr_bits else np.uint8
        W, H = (pic_w + 63) & ~63, (pic_h + 63) & ~63
        qm = np.ascontiguousarray(qt.qm)
        qmi = np.ascontiguousarray(qt.qm_inv)
        ldq = [np.zeros((H, W), np.int32) for _ in range(5)]
        recon = []
        blocks = 0
        for pli in range(3):
            p = 1 if pli else 0
            qm_off, qb, bb = _tables(qt, pli)
            px = np.zeros((H, W), pdt)
            rec = [np.zeros((H, W), pdt) for _ in range(5)]
            rec_arr = (ctypes.c_void_p * 5)(*[a.ctypes.data for a in rec])
            if decisions is not None:
                dump = []
                for bs in range(5):
                    n = 4 << bs
                    nblk = (H // n) * (W // n)
                    dump.append((np.zeros((nblk, min(n * n, 512)), np.int32),
                                 np.zeros((nblk, NBANDS[bs], 4), np.int32)))
                ytab = (ctypes.c_void_p * 5)(*[d[0].ctypes.data for d in dump])
                btab = (ctypes.c_void_p * 5)(*[d[1].ctypes.data for d in dump])
                r.ref_stage_set_dump(ytab, btab)
                decisions.append(dump)
            _pad(px, np.ascontiguousarray(pics[pli]), fpr_bits)
            args = (P(px), W, W, H, 0, pic_w, pic_h, p, P(qm), P(qmi), qm_off, qb, bb, ctypes.c_double(lam), rec_arr)
            if inter_pred is not None:
                ppx = np.zeros((H, W), pdt)
                _pad(ppx, np.ascontiguousarray(inter_pred[pli]), fpr_bits)
                plev = [np.zeros((H, W), np.int32) for _ in range(5)]
                r.ref_forward_pyramid_plane((ctypes.c_void_p * 5)(*[a.ctypes.data for a in plev]),
                                            P(np.zeros((H, W), np.int32)), P(ppx), W, W, H, 0, pic_w, pic_h)
                blocks += r.ref_stage_plane_levels(*args, None, (ctypes.c_void_p * 5)(*[a.ctypes.data for a in plev]))
            elif pli == 0:
                blocks += r.ref_stage_plane_levels(*args, (ctypes.c_void_p * 5)(*[a.ctypes.data for a in ldq]), None)
            elif chroma_cfl:
                # the copy branch: chroma level bs predicted from luma level bs, block for block
                blocks += r.ref_stage_plane_levels(*args, None, (ctypes.c_void_p * 5)(*[a.ctypes.data for a in ldq]))
            else:
                blocks += r.ref_stage_plane_levels(*args, None, None)
            if decisions is not None:
                r.ref_stage_set_dump(None, None)
            recon.append(rec)
        return recon, blocks
    finally:
        r.ref_set_fpr(0)
        r.ref_stage_set_inter(0)
        r.ref_stage_set_dump(None, None)


def stack444(frames):
    """[[Y, Cb, Cr]] * F -> (luma [F][h][w], chroma [2F][h][w]: all Cb, then all Cr)."""
    luma = np.stack([f[0] for f in frames])
    chroma = np.concatenate([np.stack([f[1] for f in frames]), np.stack([f[2] for f in frames])])
    return np.ascontiguousarray(luma), np.ascontiguousarray(chroma)


def gpu_pipe444(D, qt, frames, pic_w, pic_h, inter_pred=None, **kw):
    """A chroma_444 pipe holding `frames` ([[Y, Cb, Cr]] * F) and, for inter pipes, the
    prediction pictures inter_pred (same form)."""
    pipe = D.Pipe(qt, len(frames), pic_w, pic_h, chroma_444=True, inter=inter_pred is not None, **kw)
    try:
        assert pipe.chroma_levels == 5
        pipe.set_pictures(*stack444(frames))
        if inter_pred is not None:
            pipe.set_reference_pictures(*stack444(inter_pred))
    except BaseException:
        pipe.destroy()
        raise
    return pipe


def recon444(D, pipe):
    """recon[set][bs] of the last step: [nplanes][H][W] (uint16 with fpr_bits)."""
    rdt = np.uint16 if pipe.fpr_bits else np.uint8
    F, W, H = pipe.frames, pipe.W, pipe.H
    return [[pipe.read(D.BUF_RECON, s, bs, dtype=rdt).reshape(F * (1 + s), H, W) for bs in range(5)]
            for s in (0, 1)]


def compare_frame444(gpu, cpu, frame=0, frames=1):
    """(plane, level, differing pixels) of picture `frame`; empty = bit-exact."""
    bad = []
    for pli in range(3):
        s = 1 if pli else 0
        plane = frame if pli == 0 else (pli - 1) * frames + frame
        for bs in range(5):
            d = int(np.count_nonzero(gpu[s][bs][plane] != cpu[pli][bs]))
            if d:
                bad.append((pli, bs, d))
    return bad


def decisions444(D, pipe):
    """{(set, level): (y int32 [B][len], band int32 [B][nb][4], coded bool [B][nb])} of the last
    step, read from the choice records and the pulse slots they name (the fields the inverse
    consumes); chroma at all five levels."""
    out = {}
    for s in (0, 1):
        with_ref = pipe.inter or bool(s and pipe.chroma_cfl)
        for bs in range(5):
            nb, offs, ln = D.pvq_band_layout(bs)
            B = pipe.nblocks(s, bs)
            ych = np.zeros((B, ln), np.int32)
            band = np.zeros((B, nb, 4), np.int32)
            coded = np.zeros((B, nb), bool)
            yall = pipe.read(D.BUF_Y, s, bs, dtype=np.int16)
            if with_ref:
                ch = pipe.read(D.BUF_CHOICE, s, bs, dtype=np.int32).reshape(B, nb, 16)
                y = yall.reshape(-1, B, ln)
                for i in range(nb):
                    a, b = offs[i], offs[i + 1]
                    noref, skip, slot = ch[:, i, 2], ch[:, i, 6], ch[:, i, 9]
                    band[:, i, 0] = ch[:, i, 7]
                    band[:, i, 1] = ch[:, i, 3]
                    band[:, i, 2] = ch[:, i, 4]
                    band[:, i, 3] = ch[:, i, 5]
                    idx = np.nonzero((skip == 0) & (slot >= 0))[0]
                    v = y[slot[idx], idx, a:b].astype(np.int32)
                    v[noref[idx] == 0, -1] = 0       # a theta winner holds n - 1 pulses
                    ych[idx, a:b] = v
                    coded[:, i] = skip == 0
            else:
                ch = pipe.read(D.BUF_CHOICE, s, bs, dtype=np.int32).reshape(B, nb, 4)
                y = yall.reshape(2, B, ln)
                for i in range(nb):
                    a, b = offs[i], offs[i + 1]
                    sel, qg = ch[:, i, 0], ch[:, i, 1]
                    band[:, i, 0] = qg
                    band[:, i, 1] = -1
                    idx = np.nonzero(qg != 0)[0]
                    ych[idx, a:b] = y[sel[idx], idx, a:b]
                    band[:, i, 3] = np.abs(ych[:, a:b]).sum(axis=1)
                    coded[:, i] = True
            out[(s, bs)] = (ych, band, coded)
    return out


def compare_decisions444(gpu, cpu, frame=0, frames=1):
    """gpu: decisions444(); cpu: the `decisions` list of cpu_frame444() for picture `frame`.
    (plane, level, what, count) mismatches; empty = every gain index, theta, K and pulse equal."""
    import daala_amd as D
    bad = []
    for pli in range(3):
        s = 1 if pli else 0
        plane = frame if pli == 0 else (pli - 1) * frames + frame
        for bs, (yc, bc) in enumerate(cpu[pli]):
            yg, bg, coded = gpu[(s, bs)]
            per = yc.shape[0]
            sl = slice(plane * per, (plane + 1) * per)
            yg, bg, coded = yg[sl], bg[sl], coded[sl]
            d = int(np.count_nonzero((bg != bc).any(axis=2)))
            if d:
                bad.append((pli, bs, "band", d))
            nb, offs, _ = D.pvq_band_layout(bs)
            for i in range(nb):
                a, b = offs[i], offs[i + 1]
                on = coded[:, i]
                d = int(np.count_nonzero((yg[on, a:b] != yc[on, a:b]).any(axis=1)))
                if d:
                    bad.append((pli, bs, "y[band %d]" % i, d))
    return bad


def time_steps(D, pipe, steps, warmup, repeats):
    """bench.py's way: warm-up steps, then `repeats` timed runs of `steps` steps + flush + sync;
    the median milliseconds per step."""
    for _ in range(warmup):
        pipe.step()
    pipe.flush()
    pipe.sync()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            pipe.step()
        pipe.flush()
        pipe.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    return float(np.median(ms))
