"""Host restatement of the synchronisation layer's geometry fit (wmar/watermarking/synchronization.py:90-201) and positions step
(:224-243) in numpy + scipy: what wmar_amd/csrc/sync.hip computes, written independently of it.  `spline_rotate_values` restates
scipy.ndimage.rotate(order=3, mode="constant", reshape=False) without scipy, the way the kernels evaluate it (prefilter once per
mask, 4 x 4 taps per output pixel); tests/test_sync_reference.py holds it against scipy."""
import math

import numpy as np

ANGLES = np.arange(-20, 21)
MSGS = np.array([[0] * 32, [0] * 16 + [1] * 16, [1] * 16 + [0] * 16, [1] * 32], dtype=np.int64)
POLE = math.sqrt(3.0) - 2.0


def labels_of(positions):
    """1..4 for positions 0..3, 0 for the rest (-1 and anything else)."""
    wm = np.zeros(positions.shape, dtype=np.int64)
    for k in range(4):
        wm[positions == k] = k + 1
    return wm


def rotate_wm(wm, angle):
    from scipy import ndimage
    res = np.zeros_like(wm)
    for i in range(1, 5):
        res[ndimage.rotate((wm == i) * 255, angle, reshape=False) >= 0.5] = i
    return res


# ---- scipy's cubic spline rotation without scipy ------------------------------------------------------------------------------
def spline_prefilter_1d(c):
    """In-place cubic B-spline prefilter along axis 0 of `c` (fp64), mirror initialisation (what mode="constant" uses)."""
    n, z = c.shape[0], POLE
    c *= (1.0 - z) * (1.0 - 1.0 / z)
    zn1 = z ** (n - 1)
    acc = c[0] + zn1 * c[n - 1]
    zi = z
    for i in range(1, n - 1):
        acc = acc + zi * (c[i] + zn1 * c[n - 1 - i])
        zi *= z
    c[0] = acc / (1.0 - zn1 * zn1)
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def spline_coefficients(mask):
    c = mask.astype(np.float64).copy()
    spline_prefilter_1d(c)              # axis 0
    spline_prefilter_1d(c.T)            # axis 1 (a view: in place)
    return c


def _weights(t):
    """Cubic B-spline weights of the taps floor(x) - 1 .. floor(x) + 2 for the fraction t = x - floor(x)."""
    z = 1.0 - t
    w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    w0 = z * z * z / 6.0
    return w0, w1, w2, 1.0 - w0 - w1 - w2


def _mirror(i, n):
    """Index of tap `i` of a length-`n` line: whole-sample mirror about 0 and n - 1."""
    i = np.where(i < 0, -i, i)
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def spline_rotate_values(coeffs, angle):
    """The fp64 values scipy interpolates for every output pixel before it rounds them (0 outside the input's extent)."""
    S = coeffs.shape[0]
    r = math.radians(float(angle))
    c, s = math.cos(r), math.sin(r)
    ctr = (S - 1) / 2.0
    off0, off1 = ctr - (c * ctr + s * ctr), ctr - (-s * ctr + c * ctr)
    i, j = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    y = i * c + j * s + off0
    x = i * (-s) + j * c + off1
    inside = (y >= 0) & (y <= S - 1) & (x >= 0) & (x <= S - 1)
    y, x = np.where(inside, y, 0.0), np.where(inside, x, 0.0)
    fy, fx = np.floor(y), np.floor(x)
    wy, wx = _weights(y - fy), _weights(x - fx)
    out = np.zeros((S, S))
    for a in range(4):
        iy = _mirror(fy.astype(np.int64) - 1 + a, S)
        for b in range(4):
            ix = _mirror(fx.astype(np.int64) - 1 + b, S)
            out += coeffs[iy, ix] * wy[a] * wx[b]
    return np.where(inside, out, 0.0)


# ---- the fit --------------------------------------------------------------------------------------------------------------------
def find_cut(cumsums, pairs, dim, SZ, seen=None):
    """`seen` (a set, optional) collects the names of the branches taken: the census of tests/test_sync_reference.py."""
    cut, cut_weight, votes = 0, 0, 0
    for l, r in pairs:
        cl, cr = cumsums[dim][l], cumsums[dim][r]
        normal = cr + (cl[-1] - cl)
        flipped = cl + (cr[-1] - cr)
        idx_n = np.where(normal == normal.min())[0]
        idx_f = np.where(flipped == flipped.min())[0]
        if (normal.min() - len(idx_n) * 1e-3 < flipped.min() - len(idx_f) * 1e-3) or dim == 1:
            is_f, idx = False, idx_n
            votes -= 1
        else:
            is_f, idx = True, idx_f
            votes += 1
        if cr[-1] != 0 and cl[-1] == 0:
            pick, branch = (idx[0] if is_f else idx[-1]), "only_R"
        elif cl[-1] != 0 and cr[-1] == 0:
            pick, branch = (idx[-1] if is_f else idx[0]), "only_L"
        else:
            pick, branch = (idx[0] + idx[-1]) // 2, "both" if cl[-1] != 0 else "neither"
        if seen is not None:
            seen.add(f"{branch}_{'flipped' if is_f else 'normal'}_curve")
        w = int(cl[-1] + cr[-1])
        cut += int(pick) * w
        cut_weight += w
    if cut_weight == 0:
        if seen is not None:
            seen.add("no_weight")
        return 1e9, SZ // 2, False
    if seen is not None:
        if (2 * cut) % cut_weight == 0 and (2 * cut // cut_weight) % 2 == 1:
            seen.add("half_cut_floor_even" if (cut // cut_weight) % 2 == 0 else "half_cut_floor_odd")
        if votes == 0 and dim == 0:
            seen.add("votes_zero_dim0")
    cut = round(cut / cut_weight)
    flipped_vote = (votes / cut_weight) > 0
    error = 0
    for l, r in pairs:
        cl, cr = cumsums[dim][l], cumsums[dim][r]
        error += int((cl + (cr[-1] - cr))[cut] if flipped_vote else (cr + (cl[-1] - cl))[cut])
    return error, cut, flipped_vote


def fit_angle(wm_rot, seen=None):
    S = wm_rot.shape[-1]
    thresh = 40 if S == 256 else 80
    cumsums = [[None], [None]]
    for dim in range(2):
        for i in range(1, 5):
            sums = np.sum(wm_rot == i, axis=dim)
            if seen is not None:                         # axis 0 sums over the rows: one count per column
                for v, what in ((thresh, "on_thresh"), (thresh - 1, "below_thresh")):
                    if np.any(sums == v):
                        seen.add(f"{'column' if dim == 0 else 'row'}_count_{what}")
            sums[sums < thresh] = 0
            cumsums[dim].append(np.cumsum(sums))
    errori, cuti, _ = find_cut(cumsums, [(1, 3), (2, 4)], 1, S, seen)
    errorj, cutj, flipped = find_cut(cumsums, [(1, 2), (3, 4)], 0, S, seen)
    return float(errori + errorj), cuti, cutj, flipped


def fit_detail(positions, rotate=rotate_wm, seen=None):
    """((rotation, cut_i, cut_j, flipped), total_error fp64 [41], cuts int32 [41, 3] = (cut_i, cut_j, flipped) of every angle)."""
    S = positions.shape[-1]
    wm = labels_of(positions)
    best, best_angles, total = (float("inf"), S // 2, S // 2, False), [0], np.zeros(len(ANGLES))
    cuts = np.zeros((len(ANGLES), 3), dtype=np.int32)
    for n, angle in enumerate(ANGLES):
        e, ci, cj, fl = fit_angle(rotate(wm, angle), seen)
        total[n] = e
        cuts[n] = (ci, cj, int(fl))
        if e < best[0]:
            best, best_angles = (e, ci, cj, fl), [int(angle)]
        elif e == best[0]:
            best_angles.append(int(angle))
    if seen is not None:
        seen.add("several_best_angles" if len(best_angles) > 1 else "one_best_angle")
        if (max(best_angles) + min(best_angles)) % 2:
            seen.add("half_rotation")
    rotation = round((max(best_angles) + min(best_angles)) / 2)
    return (rotation, int(best[1]), int(best[2]), bool(best[3])), total, cuts


def fit(positions, rotate=rotate_wm):
    """((rotation, cut_i, cut_j, flipped), total_error fp64 [41]) of one label map."""
    return fit_detail(positions, rotate)[:2]


class PlainRotator:
    """rotate_wm through spline_rotate_values instead of scipy, the four prefilters run once per map (they do not depend on the
    angle): `PlainRotator()(wm, angle)`."""

    def __init__(self):
        self.key, self.coeffs = None, None

    def __call__(self, wm, angle):
        if self.key is None or self.key is not wm:
            self.key, self.coeffs = wm, [spline_coefficients((wm == i) * 255) for i in range(1, 5)]
        res = np.zeros_like(wm)
        for i in range(1, 5):
            res[spline_rotate_values(self.coeffs[i - 1], angle) >= 0.5] = i
        return res


def source_coordinates(S, angle):
    """fp64 (y, x) [S, S] of the input point every output pixel of a rotation by `angle` degrees samples."""
    r = math.radians(float(angle))
    c, s = math.cos(r), math.sin(r)
    ctr = (S - 1) / 2.0
    off0, off1 = ctr - (c * ctr + s * ctr), ctr - (-s * ctr + c * ctr)
    i, j = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    return i * c + j * s + off0, i * (-s) + j * c + off1


def rotate_wm_plain(wm, angle):
    """rotate_wm through spline_rotate_values instead of scipy."""
    res = np.zeros_like(wm)
    for i in range(1, 5):
        res[spline_rotate_values(spline_coefficients((wm == i) * 255), angle) >= 0.5] = i
    return res


# ---- positions --------------------------------------------------------------------------------------------------------------------
def positions_from_preds(preds):
    """(positions int8 [S, S], sizes int32 [4]) of one fp32 [33, S, S] prediction."""
    import torch
    p = torch.from_numpy(np.ascontiguousarray(preds))
    bits = (p[1:] > 0).long().numpy()
    dists = np.abs(bits[None] - MSGS[:, :, None, None]).sum(axis=1)       # [4, S, S]
    idx = dists.argmin(axis=0)
    keep = (dists.min(axis=0) <= 6) & (torch.sigmoid(p[0]) > 0.5).numpy()
    pos = np.where(keep, idx, -1).astype(np.int8)
    return pos, np.array([(pos == k).sum() for k in range(4)], dtype=np.int32)


def gate_fails(sizes, S):
    return int(np.sum(sizes)) < round(S * S * (0.7 if S == 256 else 0.75))
