"""Integer numpy restatement of what PIL's `save(format="JPEG", quality=q)` followed by `Image.open(...).convert("RGB")` does to the
pixels of an RGB image whose height and width are multiples of 16 (libjpeg-turbo's default baseline path; entropy coding is lossless,
so the decoded pixels are an integer function of the input pixels and q):

  jccolor.c   RGB -> YCbCr, 16-bit fixed point
  jcsample.c  h2v2_downsample: 2 x 2 box sums of Cb / Cr, bias 1, 2, 1, 2, ... along each output row
  jfdctint.c  jpeg_fdct_islow on sample - 128 (rows, then columns)
  jcdctmgr.c  quantisation by 8 t, rounded half away from zero
  jidctint.c  jpeg_idct_islow on k t (columns, then rows), post-IDCT range-limit table
  jdsample.c  h2v2_fancy_upsample (triangle filter, edge rows / columns replicated)
  jdcolor.c   YCbCr -> RGB, 16-bit fixed point, clamped to [0, 255]

Quantisation tables: ITU T.81 Annex K, scaled as jcparam.c jpeg_set_quality(q, force_baseline=TRUE).  The kernel of
wmar_amd/csrc/jpeg.hip is written against this restatement; tests/test_jpeg_integer_pipeline.py pins it to PIL bit for bit."""
import numpy as np

STD_LUMINANCE = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
    103, 99], dtype=np.int64).reshape(8, 8)
STD_CHROMINANCE = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32, dtype=np.int64).reshape(8, 8)

CONST_BITS, PASS1_BITS = 13, 2
F0298, F0390, F0541, F0765, F0899, F1175 = 2446, 3196, 4433, 6270, 7373, 9633
F1501, F1847, F1961, F2053, F2562, F3072 = 12299, 15137, 16069, 16819, 20995, 25172


def _fix16(x):
    return int(x * 65536 + 0.5)


def quant_tables(q):
    """(luminance, chrominance) 8 x 8 tables of jpeg_set_quality(q, TRUE)."""
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * s + 50) // 100, 1, 255) for t in (STD_LUMINANCE, STD_CHROMINANCE))


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """one pass of jpeg_fdct_islow over the last axis of d (8 entries)"""
    d = [d[..., i] for i in range(8)]
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    sh = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    o = [None] * 8
    if first:
        o[0], o[4] = (tmp10 + tmp11) << PASS1_BITS, (tmp10 - tmp11) << PASS1_BITS
    else:
        o[0], o[4] = _descale(tmp10 + tmp11, PASS1_BITS), _descale(tmp10 - tmp11, PASS1_BITS)
    z1 = (tmp12 + tmp13) * F0541
    o[2], o[6] = _descale(z1 + tmp13 * F0765, sh), _descale(z1 - tmp12 * F1847, sh)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * F1175
    tmp4, tmp5, tmp6, tmp7 = tmp4 * F0298, tmp5 * F2053, tmp6 * F3072, tmp7 * F1501
    z1, z2, z3, z4 = -z1 * F0899, -z2 * F2562, -z3 * F1961 + z5, -z4 * F0390 + z5
    o[7], o[5] = _descale(tmp4 + z1 + z3, sh), _descale(tmp5 + z2 + z4, sh)
    o[3], o[1] = _descale(tmp6 + z2 + z3, sh), _descale(tmp7 + z1 + z4, sh)
    return np.stack(o, axis=-1)


def _idct_1d(d, first):
    """one pass of jpeg_idct_islow over the last axis of d (8 entries); the second pass returns range-limit indices"""
    d = [d[..., i] for i in range(8)]
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * F0541
    tmp2, tmp3 = z1 - z3 * F1847, z1 + z2 * F0765
    tmp0, tmp1 = (d[0] + d[4]) << CONST_BITS, (d[0] - d[4]) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F1175
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F0298, tmp1 * F2053, tmp2 * F3072, tmp3 * F1501
    z1, z2, z3, z4 = -z1 * F0899, -z2 * F2562, -z3 * F1961 + z5, -z4 * F0390 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    sh = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS + 3
    o = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([_descale(v, sh) for v in o], axis=-1)


def range_limit(x):
    """the decoder's post-IDCT table, indexed by x & 1023"""
    v = x & 1023
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896)))


def code_plane(plane, table):
    """[h, w] samples (h, w multiples of 8) -> the decoder's reconstruction of them"""
    h, w = plane.shape
    blk = (plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3) - 128).astype(np.int64)
    c = _fdct_1d(_fdct_1d(blk, True).swapaxes(-1, -2), False).swapaxes(-1, -2)        # rows, then columns
    d = 8 * table
    a = np.abs(c) + d // 2
    k = np.sign(c) * np.where(a >= d, a // d, 0)
    r = _idct_1d(_idct_1d((k * table).swapaxes(-1, -2), True).swapaxes(-1, -2), False)  # columns, then rows
    return range_limit(r).transpose(0, 2, 1, 3).reshape(h, w)


def fancy_upsample(c):
    """h2v2_fancy_upsample of a [h, w] chroma plane -> [2h, 2w]"""
    up, down = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    cs = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
    cs[0::2], cs[1::2] = 3 * c + up, 3 * c + down
    left, right = np.concatenate([cs[:, :1], cs[:, :-1]], 1), np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
    out = np.empty((cs.shape[0], 2 * cs.shape[1]), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * cs + left + 8) >> 4, (3 * cs + right + 7) >> 4
    out[:, 0], out[:, -1] = (4 * cs[:, 0] + 8) >> 4, (4 * cs[:, -1] + 7) >> 4
    return out


def roundtrip(rgb, q):
    """[H, W, 3] uint8 (H, W multiples of 16) -> [H, W, 3] uint8, the pixels PIL decodes after encoding at quality q"""
    H, W, _ = rgb.shape
    assert H % 16 == 0 and W % 16 == 0 and 1 <= q <= 100
    R, G, B = (rgb[..., i].astype(np.int64) for i in range(3))
    f = _fix16
    Y = (f(0.299) * R + f(0.587) * G + f(0.114) * B + (1 << 15)) >> 16
    Cb = (-f(0.16874) * R - f(0.33126) * G + f(0.5) * B + (128 << 16) + (1 << 15) - 1) >> 16
    Cr = (f(0.5) * R - f(0.41869) * G - f(0.08131) * B + (128 << 16) + (1 << 15) - 1) >> 16
    bias = 1 + (np.arange(W // 2) & 1)
    ds = [(P[0::2, 0::2] + P[0::2, 1::2] + P[1::2, 0::2] + P[1::2, 1::2] + bias) >> 2 for P in (Cb, Cr)]
    tl, tc = quant_tables(q)
    y = code_plane(Y, tl)
    cb, cr = (fancy_upsample(code_plane(P, tc)) - 128 for P in ds)
    r = y + ((f(1.402) * cr + (1 << 15)) >> 16)
    b = y + ((f(1.772) * cb + (1 << 15)) >> 16)
    g = y + ((-f(0.71414) * cr - f(0.34414) * cb + (1 << 15)) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def pil_roundtrip(rgb, q):
    """the same through PIL (libjpeg-turbo)"""
    import io

    from PIL import Image
    with io.BytesIO() as buf:
        Image.fromarray(rgb).save(buf, format="JPEG", quality=q)
        buf.seek(0)
        return np.asarray(Image.open(buf).convert("RGB"))
