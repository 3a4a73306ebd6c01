"""Readers for the decision-export tests (tests/test_gpu_export_ring.py, tests/test_gpu_export_inter.py) - TEST
INFRASTRUCTURE.

decisions()      what the pipe's last step decided for every band of every block, read from the dense device
                 buffers: the choice records and the pulse slot each record names - 16 ints per band
                 {.., [2] noref, [3] itheta, [4] max_theta, [5] k, [6] skip, [7] coded gain index, .., [9] slot}
                 for the planes coded against a reference (keyframe chroma with chroma from luma, EVERY plane of
                 an inter step), 4 ints {slot, gain index, ..} for keyframe luma.  4:2:0 and 4:4:4 (chroma at
                 pipe.chroma_levels levels).  Same form as daala_amd.Pipe.decode_export.
export_diff()    the mismatches between a decoded export and decisions().
export_flags()   the no-reference and skip flags of an export buffer; dense_flags() the same from the device.
pictures()       [Y, Cb, Cr] pictures of a given size and chroma decimation from the bench generators."""
import numpy as np


def pictures(content, index, seed, pw, ph, chroma_444=False):
    import bench
    if chroma_444:
        import _pipe444_check as C4
        return C4.pictures444(content, index, seed, pw, ph)
    fr = bench.CONTENT[content](index, seed)
    return [np.ascontiguousarray(fr[0][:ph, :pw])] + [np.ascontiguousarray(p[:ph // 2, :pw // 2]) for p in fr[1:]]


def stack(frames):
    """[[Y, Cb, Cr]] * F -> (luma [F][h][w], chroma [2F][ch][cw]: all Cb, then all Cr)."""
    luma = np.stack([f[0] for f in frames])
    chroma = np.concatenate([np.stack([f[1] for f in frames]), np.stack([f[2] for f in frames])])
    return np.ascontiguousarray(luma), np.ascontiguousarray(chroma)


def _with_ref(D, pipe, set_, bs, B, nb, offs, ln):
    ch = pipe.read(D.BUF_CHOICE, set_, bs, dtype=np.int32).reshape(B, nb, 16)
    y = pipe.read(D.BUF_Y, set_, bs, dtype=np.int16).reshape(-1, B, ln)
    ych = np.zeros((B, ln), np.int32)
    band = np.zeros((B, nb, 4), np.int32)
    coded = np.zeros((B, nb), bool)
    for i in range(nb):
        a, b = offs[i], offs[i + 1]
        noref, skip, slot = ch[:, i, 2], ch[:, i, 6], ch[:, i, 9]
        band[:, i, 0] = ch[:, i, 7]
        band[:, i, 1] = ch[:, i, 3]
        band[:, i, 2] = ch[:, i, 4]
        band[:, i, 3] = ch[:, i, 5]
        idx = np.nonzero((skip == 0) & (slot >= 0))[0]
        v = y[slot[idx], idx, a:b].astype(np.int32)
        v[noref[idx] == 0, -1] = 0       # a theta winner holds n - 1 pulses (src/pvq_encoder.c:530)
        ych[idx, a:b] = v
        coded[:, i] = skip == 0
    return ych, band, coded


def _noref(D, pipe, set_, bs, B, nb, offs, ln):
    ch = pipe.read(D.BUF_CHOICE, set_, bs, dtype=np.int32).reshape(B, nb, 4)
    y = pipe.read(D.BUF_Y, set_, bs, dtype=np.int16).reshape(2, B, ln)
    ych = np.zeros((B, ln), np.int32)
    band = np.zeros((B, nb, 4), np.int32)
    for i in range(nb):
        a, b = offs[i], offs[i + 1]
        sel, qg = ch[:, i, 0], ch[:, i, 1]
        band[:, i, 0] = qg
        band[:, i, 1] = -1
        idx = np.nonzero(qg != 0)[0]
        ych[idx, a:b] = y[sel[idx], idx, a:b]
        band[:, i, 3] = np.abs(ych[:, a:b]).sum(axis=1)
    return ych, band, np.ones((B, nb), bool)


def decisions(D, pipe):
    """{(set, level): (y int32 [B][len], band int32 [B][nb][4] = {coded gain index, itheta, max_theta, k},
    coded bool [B][nb])} of the pipe's last step (sync first)."""
    out = {}
    for s in (0, 1):
        for bs in range(5 if s == 0 else pipe.chroma_levels):
            nb, offs, ln = D.pvq_band_layout(bs)
            B = pipe.nblocks(s, bs)
            ref = pipe.inter or (s == 1 and pipe.chroma_cfl)
            out[(s, bs)] = (_with_ref if ref else _noref)(D, pipe, s, bs, B, nb, offs, ln)
    return out


def export_diff(got, want):
    """(key, what) of every section whose decoded export differs from decisions(): gain index, theta and its range,
    the skip flag, K of the coded bands, every pulse.  Empty = equal."""
    bad = []
    if set(got) != set(want):
        return [("sections", sorted(set(got) ^ set(want)))]
    for key in sorted(want):
        yw, bw, cw = want[key]
        yg, bg, cg = got[key]
        if not np.array_equal(cg, cw):
            bad.append((key, "coded"))
        if not np.array_equal(bg[..., :3], bw[..., :3]):
            bad.append((key, "gain index / theta / max_theta"))
        if not np.array_equal(bg[..., 3][cw], bw[..., 3][cw]):
            bad.append((key, "K of the coded bands"))
        if not np.array_equal(yg, yw):
            bad.append((key, "pulses"))
    return bad


def export_flags(host, lay):
    """{section: (noref bool [records], skip int [records])} of an export buffer (bits 9 and 10-11 of `fn`)."""
    out = {}
    for si, sec in enumerate(lay["sections"]):
        rb = sec["record_bytes"]
        rec = host[sec["records_off"]:sec["records_off"] + sec["nrecords"] * rb].view(np.uint16).reshape(-1, rb // 2)
        fn = rec[:, -1].astype(np.int64)
        out[si] = ((fn >> 9 & 1).astype(bool), fn >> 10 & 3)
    return out


def dense_flags(D, pipe):
    """The same flags from the choice records of the with-reference planes: {section: (noref, skip)}."""
    out = {}
    si = 0
    for s in (0, 1):
        for bs in range(5 if s == 0 else pipe.chroma_levels):
            if pipe.inter or (s == 1 and pipe.chroma_cfl):
                nb, _, _ = D.pvq_band_layout(bs)
                ch = pipe.read(D.BUF_CHOICE, s, bs, dtype=np.int32).reshape(-1, 16)
                out[si] = (ch[:, 2] != 0, ch[:, 6].astype(np.int64) & 3)
            si += 1
    return out
