"""The yardstick of the Haar-wavelet path: the reference's own loops, restated on Python integers.

Every function cites the lines it restates.  The shape is the reference's - a block at a time, the transform first, the
quantiser's two loops, the recursive tree, the raster DC walk - and deliberately not the fused level-by-level sweep of
daala_amd/csrc/haar_kernels.hip.  tests/test_haar_ref.py pins haar / haar_inv to the compiled reference.

Blocks are lists of rows of Python ints (no wrap-around to hide), planes numpy arrays."""
import numpy as np

OD_COEFF_SHIFT = 4                                   # src/internal.h:124
# src/state.c:55-60: per decomposition level, starting from LF
OD_HAAR_QM = ((16, 16, 16, 16, 24, 32), (16, 16, 16, 24, 32, 48))


def haar_kernel(ll, lh, hl, hh):
    """OD_HAAR_KERNEL, src/tf.h:34-45."""
    ll += hl
    hh -= lh
    llmhh_2 = (ll - hh) >> 1
    lh = llmhh_2 - lh
    hl = llmhh_2 - hl
    ll -= lh
    hh += hl
    return ll, lh, hl, hh


def haar(x, ln):
    """od_haar, src/dct.c:4822-4859."""
    n = 1 << ln
    tmp = [[int(x[i][j]) for j in range(n)] for i in range(n)]
    y = [[0] * n for _ in range(n)]
    for level in range(ln):
        npairs = n >> level >> 1
        for i in range(npairs):
            for j in range(npairs):
                a = tmp[2 * i][2 * j]
                b = tmp[2 * i + 1][2 * j]
                c = tmp[2 * i][2 * j + 1]
                d = tmp[2 * i + 1][2 * j + 1]
                a, b, c, d = haar_kernel(a, b, c, d)
                tmp[i][j] = a
                y[i][j + npairs] = b
                y[i + npairs][j] = c
                y[i + npairs][j + npairs] = d
    y[0][0] = tmp[0][0]
    return y


def haar_inv(y, ln):
    """od_haar_inv, src/dct.c:4861-4888."""
    n = 1 << ln
    x = [[0] * n for _ in range(n)]
    x[0][0] = int(y[0][0])
    for level in range(ln - 1, -1, -1):
        npairs = 1 << (ln - 1 - level)
        for i in range(npairs - 1, -1, -1):
            for j in range(npairs - 1, -1, -1):
                a = x[i][j]
                b = int(y[i][j + npairs])
                c = int(y[i + npairs][j])
                d = int(y[i + npairs][j + npairs])
                a, b, c, d = haar_kernel(a, b, c, d)
                x[2 * i][2 * j] = a
                x[2 * i + 1][2 * j] = b
                x[2 * i][2 * j + 1] = c
                x[2 * i + 1][2 * j + 1] = d
    return x


def div_r0(x, y):
    """OD_DIV_R0, src/odintrin.h:123, with C's division (towards zero)."""
    off = ((y + 1) >> 1) - 1
    num = x - off if x < 0 else x + off              # OD_FLIPSIGNI(off, x)
    return -(-num // y) if num < 0 else num // y


def compute_max_tree(tree_sum, x, y, c, ln):
    """od_compute_max_tree, src/encode.c:899-919."""
    n = 1 << ln
    maxval = 0
    if 2 * x < n and 2 * y < n:
        maxval += compute_max_tree(tree_sum, 2 * x, 2 * y, c, ln)
        maxval += compute_max_tree(tree_sum, 2 * x + 1, 2 * y, c, ln)
        maxval += compute_max_tree(tree_sum, 2 * x, 2 * y + 1, c, ln)
        maxval += compute_max_tree(tree_sum, 2 * x + 1, 2 * y + 1, c, ln)
    maxval += abs(c[y][x])
    tree_sum[y][x] = maxval
    return maxval


def subband_q(quant, direction, level):
    """src/encode.c:1018-1019."""
    return 1 if quant == 0 else quant * OD_HAAR_QM[direction == 2][level] >> 4


def wavelet_quantize(dblock, predt, ln, quant, stats=None):
    """od_wavelet_quantize, src/encode.c:1003-1080, without its entropy coder: (the quantised block with [0][0] as
    found, tree_sum, the dequantised block with [0][0] as found)."""
    n = 1 << ln
    out = [[0] * n for _ in range(n)]
    out[0][0] = dblock[0][0]
    for direction in range(3):
        for level in range(ln):
            by = ((direction + 1) >> 1) << level     # bo of :1017, as a row and a column
            bx = ((direction + 1) & 1) << level
            q = subband_q(quant, direction, level)
            for i in range(1 << level):
                for j in range(1 << level):
                    num = dblock[by + i][bx + j] - predt[by + i][bx + j]
                    out[by + i][bx + j] = div_r0(num, q)
                    if stats is not None and q % 2 == 0 and abs(num) % q == q // 2:
                        stats["ties_neg" if num < 0 else "ties_pos"] += 1
    tree_sum = [[0] * n for _ in range(n)]
    compute_max_tree(tree_sum, 1, 0, out, ln)
    compute_max_tree(tree_sum, 0, 1, out, ln)
    compute_max_tree(tree_sum, 1, 1, out, ln)
    tree_sum[0][0] = tree_sum[0][1] + tree_sum[1][0] + tree_sum[1][1]       # :1033
    deq = [row[:] for row in out]
    for direction in range(3):                        # :1065-1078
        for level in range(ln):
            by = ((direction + 1) >> 1) << level
            bx = ((direction + 1) & 1) << level
            q = subband_q(quant, direction, level)
            for i in range(1 << level):
                for j in range(1 << level):
                    deq[by + i][bx + j] = q * out[by + i][bx + j] + predt[by + i][bx + j]
    return out, tree_sum, deq


def quantize_haar_dc_sb(sb_dc_mem, nhsb, bx, by, dc, dc_quant, has_ur, stats=None):
    """od_quantize_haar_dc_sb, src/encode.c:1563-1587: (the coded symbol, the reconstructed DC); sb_dc_mem updated."""
    case = "none"
    if by > 0 and bx > 0:
        if has_ur:
            case = "four"
            s = (22 * sb_dc_mem[by * nhsb + bx - 1] - 9 * sb_dc_mem[(by - 1) * nhsb + bx - 1]
                 + 15 * sb_dc_mem[(by - 1) * nhsb + bx] + 4 * sb_dc_mem[(by - 1) * nhsb + bx + 1] + 16)
        else:
            case = "three"
            s = (23 * sb_dc_mem[by * nhsb + bx - 1] - 10 * sb_dc_mem[(by - 1) * nhsb + bx - 1]
                 + 19 * sb_dc_mem[(by - 1) * nhsb + bx] + 16)
        if stats is not None and s < 0:
            stats["neg_pred_sum"] += 1
        sb_dc_pred = s >> 5
    elif by > 0:
        case = "up"
        sb_dc_pred = sb_dc_mem[(by - 1) * nhsb + bx]
    elif bx > 0:
        case = "left"
        sb_dc_pred = sb_dc_mem[by * nhsb + bx - 1]
    else:
        sb_dc_pred = 0
    if stats is not None:
        stats["dc_cases"].add(case)
    quant = div_r0(dc - sb_dc_pred, dc_quant)
    sb_dc_curr = quant * dc_quant + sb_dc_pred
    sb_dc_mem[by * nhsb + bx] = sb_dc_curr
    return quant, sb_dc_curr


def inter_dc(d0, p0, dc_quant, stats=None):
    """src/encode.c:1337-1343 and :1373-1374: (scalar_out[0] as coded, the reconstructed DC)."""
    if abs(d0 - p0) < dc_quant * 141 // 256:
        sym = 0
        if stats is not None:
            stats["dead_in"] += 1
    else:
        sym = div_r0(d0 - p0, dc_quant)
        if stats is not None:
            stats["dead_out"] += 1
    return sym, sym * dc_quant + p0


def ref_buf_to_coeff(src, lossless, depth):
    """od_ref_buf_to_coeff, src/state.c:1216-1255: uint8 planes take the 8-bit branch, int16 the FPR one."""
    s = src.astype(np.int64)
    if src.dtype == np.uint8:
        coeff_shift = depth - 8 if lossless else OD_COEFF_SHIFT      # (bitdepth_mode - OD_BITDEPTH_MODE_8)*2
        return (s - 128) * (1 << coeff_shift)
    assert src.dtype == np.int16
    coeff_shift = OD_COEFF_SHIFT - (depth - 8) if lossless else 0
    return (s - (1 << (8 + OD_COEFF_SHIFT) >> 1) + (1 << coeff_shift >> 1)) >> coeff_shift


def coeff_to_ref_buf(c, dtype, lossless, depth, stats=None):
    """od_coeff_to_ref_buf, src/state.c:1281-1323, with OD_CLAMP255 / OD_CLAMPFPR."""
    c = np.asarray(c, np.int64)
    if dtype == np.uint8:
        coeff_shift = depth - 8 if lossless else OD_COEFF_SHIFT
        v = ((c + (1 << coeff_shift >> 1)) >> coeff_shift) + 128
        top = 255
    else:
        coeff_shift = OD_COEFF_SHIFT - (depth - 8) if lossless else 0
        v = c * (1 << coeff_shift) + (128 << OD_COEFF_SHIFT)
        top = (1 << (8 + OD_COEFF_SHIFT)) - 1
    if stats is not None:
        stats["clamp_lo"] += int((v < 0).sum())
        stats["clamp_hi"] += int((v > top).sum())
    return np.clip(v, 0, top).astype(dtype)


def new_stats():
    return {"ties_pos": 0, "ties_neg": 0, "dc_cases": set(), "neg_pred_sum": 0, "dead_in": 0, "dead_out": 0,
            "zero_tree_blocks": 0, "max_tree": 0, "clamp_lo": 0, "clamp_hi": 0}


def encode_planes(px, pred, dec, pic_w, pic_h, depth, quant, dc_quant, plane_split, stats=None):
    """The coded path of a plane set the way od_encode_coefficients walks it (src/encode.c:2563-2658): px, pred
    [nplanes][h][w] (pred None: keyframe).  Returns q, tree (int32 [nplanes][h][w], the DC slots as
    include/daala_hip.h defines them), dc_rec (int32 [nplanes][nvsb*nhsb]) and rec (px's type)."""
    nplanes, h, w = px.shape
    lossless = quant == 0
    ln = 6 - dec
    n = 1 << ln
    nhsb, nvsb = w // n, h // n
    q_out = np.zeros((nplanes, h, w), np.int32)
    t_out = np.zeros((nplanes, h, w), np.int32)
    dc_out = np.zeros((nplanes, nvsb * nhsb), np.int32)
    rec_c = np.zeros((nplanes, h, w), np.int64)
    for p in range(nplanes):
        dcq = dc_quant[0] if p < plane_split else dc_quant[1]
        ctmp = ref_buf_to_coeff(px[p], lossless, depth)
        if pred is not None:
            mctmp = ref_buf_to_coeff(pred[p], lossless, depth)
            ctmp[:, pic_w:] = mctmp[:, pic_w:]                   # :2593-2597
            ctmp[pic_h:, :] = mctmp[pic_h:, :]                   # :2598-2602
        sb_dc_mem = [0] * (nvsb * nhsb)
        for sby in range(nvsb):
            for sbx in range(nhsb):
                ys, xs = slice(sby * n, (sby + 1) * n), slice(sbx * n, (sbx + 1) * n)
                dblock = haar(ctmp[ys, xs].tolist(), ln)
                if pred is None:
                    predt = [[0] * n for _ in range(n)]
                    sym, dc = quantize_haar_dc_sb(sb_dc_mem, nhsb, sbx, sby, dblock[0][0], dcq,
                                                  sby > 0 and sbx < nhsb - 1, stats)      # :2639-2640
                else:
                    predt = haar(mctmp[ys, xs].tolist(), ln)
                    sym, dc = inter_dc(dblock[0][0], predt[0][0], dcq, stats)
                    sb_dc_mem[sby * nhsb + sbx] = dc
                out, tree_sum, deq = wavelet_quantize(dblock, predt, ln, quant, stats)
                if stats is not None:
                    stats["zero_tree_blocks"] += tree_sum[0][0] == 0
                    stats["max_tree"] = max(stats["max_tree"], tree_sum[0][0])
                out[0][0] = sym
                deq[0][0] = dc
                q_out[p, ys, xs] = out
                t_out[p, ys, xs] = tree_sum
                rec_c[p, ys, xs] = haar_inv(deq, ln)
        dc_out[p] = sb_dc_mem
    rec = coeff_to_ref_buf(rec_c, px.dtype, lossless, depth, stats)
    return q_out, t_out, dc_out, rec
