"""Inputs of the synchronisation-layer tests, rebuilt from seeds (numpy only): label maps of the WAM grid layout under
nearest-neighbour index maps, seeded WAM prediction tensors, and the four images of the remove_sync end-to-end test.  The expected
outputs are recorded in tests/golden/sync_vectors.npz, those of the edge_* inputs in tests/golden/sync_edge_vectors.npz
(tests/golden/make_sync_vectors.py)."""
import numpy as np

ANGLES = np.arange(-20, 21)
ROT_ANGLES = (-20, -7, 0, 1, 20)                      # angles whose thresholded, merged map is recorded ...
ROT_CASES = ("rot+7", "flip_speckle", "random")       # ... for these 256-pixel cases
MSGS = np.array([[0] * 32, [0] * 16 + [1] * 16, [1] * 16 + [0] * 16, [1] * 32], dtype=np.int64)


def grid_positions(S):
    """Labels 0..3 in the four quadrants, -1 on the leeway cross (the layout of WamSync.create_grid_mask)."""
    pos = np.full((S, S), -1, dtype=np.int8)
    h = S // 2
    for i in range(2):
        for j in range(2):
            pos[i * h:(i + 1) * h, j * h:(j + 1) * h] = i * 2 + j
    lw = 18 if S == 256 else 36
    a, b = h - lw // 2, h + lw // 2 + 1
    pos[:, a:b] = -1
    pos[a:b, :] = -1
    return pos


def rot_index(S, angle):
    """(sy, sx, inside) of the nearest-neighbour rotation about the array centre by `angle` degrees."""
    r = np.deg2rad(angle)
    c, s = np.cos(r), np.sin(r)
    y, x = np.meshgrid(np.arange(S) - (S - 1) / 2.0, np.arange(S) - (S - 1) / 2.0, indexing="ij")
    sy = np.rint(c * y + s * x + (S - 1) / 2.0).astype(np.int64)
    sx = np.rint(-s * y + c * x + (S - 1) / 2.0).astype(np.int64)
    inside = (sy >= 0) & (sy < S) & (sx >= 0) & (sx < S)
    return np.clip(sy, 0, S - 1), np.clip(sx, 0, S - 1), inside


def rotate(a, angle, fill):
    """`a` [..., S, S] rotated by the index map, `fill` outside."""
    sy, sx, inside = rot_index(a.shape[-1], angle)
    return np.where(inside, a[..., sy, sx], np.asarray(fill, dtype=a.dtype))


def crop_resize(a, frac):
    S = a.shape[-1]
    n = int(frac * S)
    idx = np.minimum(((np.arange(S) + 0.5) * n / S).astype(np.int64), n - 1)
    return a[..., idx[:, None], idx[None, :]]


def crop_pad(a, frac, fill):
    S = a.shape[-1]
    n = int(frac * S)
    out = np.full_like(a, fill)
    out[..., :n, :n] = a[..., :n, :n]
    return out


def speckle(pos, frac, seed):
    rs = np.random.RandomState(seed)
    out = pos.copy()
    hit = rs.rand(*pos.shape) < frac
    out[hit] = rs.randint(0, 4, size=int(hit.sum())).astype(np.int8)
    return out


def _cases_256():
    g = grid_positions(256)
    left = g.copy()
    left[:, 128:] = -1
    return [
        ("identity", g),
        ("flip", g[:, ::-1].copy()),
        ("rot+2", rotate(g, 2, -1)),
        ("rot+7", rotate(g, 7, -1)),
        ("rot-13", rotate(g, -13, -1)),
        ("rot+20", rotate(g, 20, -1)),
        ("crop0.7", crop_resize(g, 0.7)),
        ("crop0.5", crop_resize(g, 0.5)),
        ("croppad0.8", crop_pad(g, 0.8, -1)),
        ("flip_speckle", speckle(g[:, ::-1].copy(), 0.01, 101)),
        ("rot-5_speckle", speckle(rotate(g, -5, -1), 0.02, 102)),
        ("all_minus1", np.full((256, 256), -1, dtype=np.int8)),
        ("left_half", left),
        ("one_label", np.where(g == 0, g, np.int8(-1)).astype(np.int8)),
        ("random", np.random.RandomState(103).randint(0, 4, size=(256, 256)).astype(np.int8)),
    ]


def label_cases(S):
    """[(name, positions int8 [S, S])] in the fixed order of the golden file."""
    if S == 256:
        return _cases_256()
    g = grid_positions(S)
    if S == 512:
        return [("flip", g[:, ::-1].copy()), ("rot-13", rotate(g, -13, -1)), ("crop0.7", crop_resize(g, 0.7))]
    if S == 128:
        return [("identity", g)]
    raise ValueError(S)


# (seed, size, layout rotation, mask-logit sign flipped): the last one fails the confidence gate
PRED_CASES = [(201, 256, 4, False), (202, 256, -6, False), (203, 256, 0, False), (204, 128, 0, True)]
PLANTED = [((10, 10), 0.0), ((10, 11), -0.0), ((10, 12), 5e-8), ((10, 13), 2e-7),
           ((200, 40), 0.0), ((200, 41), -0.0), ((200, 42), 5e-8), ((200, 43), 2e-7)]


def preds(seed, S, angle, gate_fails):
    """A seeded WAM output [33, S, S] fp32: channel 0 the mask logit (+-4, sigma 2), channels 1..32 the bit logits of the label's
    message (+-3, sigma 2.5; random bits where there is no label), with mask-logit values at the sigmoid's decision edge planted."""
    rs = np.random.RandomState(seed)
    pos = rotate(grid_positions(S), angle, -1)
    bits = np.where(pos[None] >= 0, MSGS[np.maximum(pos, 0)].transpose(2, 0, 1), rs.randint(0, 2, size=(32, S, S)))
    out = np.empty((33, S, S), dtype=np.float32)
    sign = np.where(pos >= 0, 1.0, -1.0) * (-1.0 if gate_fails else 1.0)
    out[0] = (4.0 * sign + 2.0 * rs.randn(S, S)).astype(np.float32)
    out[1:] = (3.0 * (2.0 * bits - 1.0) + 2.5 * rs.randn(32, S, S)).astype(np.float32)
    if S == 256:
        for (y, x), v in PLANTED:
            out[0, y, x] = np.float32(v)
            out[1:, y, x] = np.float32(-3.0)          # message 0 exactly: the mask decides alone
    return out


# ---- edge cases (tests/golden/sync_edge_vectors.npz): ragged sizes, every find_cut branch, ties, counts on the threshold
EDGE_FIT_SIZES = (161, 190, 257, 300, 96, 129)        # 96 and 129: no count reaches the threshold of 80, the fit is trivial
EDGE_ROT_SIZES = (4, 5, 7, 63, 64, 65, 129, 300)
EDGE_WIDE_ANGLES = (-180, -90, -45, -21, 21, 45, 90, 180)     # beyond the fit's range, recorded at 64 and 65 only
EDGE_POS_SIZES = (5, 129, 64)                         # S * S % 64 != 0 twice, then a size whose waves stay within one image


def edge_grid(S, leeway=6):
    """grid_positions with a narrow cross; at odd S the last row and column carry no label."""
    pos = np.full((S, S), -1, dtype=np.int8)
    h = S // 2
    for i in range(2):
        for j in range(2):
            pos[i * h:(i + 1) * h, j * h:(j + 1) * h] = i * 2 + j
    a, b = max(h - leeway // 2, 0), h + leeway // 2 + 1
    pos[:, a:b] = -1
    pos[a:b, :] = -1
    return pos


def edge_label_cases(S):
    """[(name, positions int8 [S, S])] in the fixed order of the golden file."""
    g = edge_grid(S)
    h = S // 2
    f = g[:, ::-1].copy()
    top, right, fleft = g.copy(), g.copy(), f.copy()
    top[h:] = -1
    right[:, :h] = -1
    fleft[:, h:] = -1
    cases = [
        ("identity", g),
        ("flip", f),
        ("rot+7", rotate(g, 7, -1)),
        ("rot-13_speckle", speckle(rotate(g, -13, -1), 0.02, 300 + S)),
        ("top_half", top),
        ("right_half", right),
        ("flip_left_half", fleft),
        ("all_minus1", np.full((S, S), -1, dtype=np.int8)),
    ]
    if S == 190:
        # turned by 7.5 degrees: the angles -8 and -7 tie, round((max + min) / 2) = round(-7.5) lands on a half whose floor is even
        cases.append(("rot+7.5", rotate(g, 7.5, -1)))
    if S == 257:
        # one row lower, and every label one row shorter so that the pair (2, 4) picks row 129 and the pair (1, 3) row 128 with
        # equal weights: the cut quotient is 128.5, a half whose floor is even (half to even: 128, half up: 129)
        e = np.full_like(g, -1)
        e[1:] = g[:-1]
        e[1, :] = -1
        e[:, 0] = -1                                    # the left quadrants as wide as the right ones: 124 columns
        e[256, :h] = -1
        e[h + 5, h:] = -1
        cases.append(("half_even", e))
    return cases


def edge_rot_angles(S):
    return ROT_ANGLES + (EDGE_WIDE_ANGLES if S in (64, 65) else ())


def edge_rot_cases():
    """[(name, positions int8 [S, S], angles)]: a map of uniform random labels -1..3 and the grid, per size."""
    out = []
    for S in EDGE_ROT_SIZES:
        rnd = np.random.RandomState(400 + S).randint(-1, 4, size=(S, S)).astype(np.int8)
        out.append((f"random{S}", rnd, edge_rot_angles(S)))
        out.append((f"grid{S}", edge_grid(S, 6 if S >= 32 else 0), edge_rot_angles(S)))
    return out


def _bits_at_distance(msg, flips, rs):
    bits = MSGS[msg].copy()
    bits[rs.choice(32, size=flips, replace=False)] ^= 1
    return bits


def edge_planted():
    """[(mask logit, bit logits fp32 [32], what)] of the planted pixels of an edge prediction tensor."""
    rs = np.random.RandomState(77)
    out = []
    for msg in range(4):                                # the Hamming gate: kept at 5 and 6 differing bits, dropped at 7
        for flips in (5, 6, 7):
            out.append((4.0, (3.0 * (2.0 * _bits_at_distance(msg, flips, rs) - 1.0)).astype(np.float32), f"msg{msg}+{flips}"))
    tiny = np.float32(np.finfo(np.float32).smallest_subnormal)
    # message 1 = 0^16 1^16 spelt with values at the edge of `logit > 0`: 0, -0 and NaN are not above 0, the smallest denormal is
    for v in (np.float32(0.0), np.float32(-0.0), np.float32(np.nan)):
        out.append((4.0, np.array([v] * 16 + [3.0] * 16, dtype=np.float32), f"zero={v}"))
    out.append((4.0, np.array([-3.0] * 16 + [tiny] * 16, dtype=np.float32), "one=denormal"))
    for v in (0.0, -0.0, 5e-8, 2e-7, np.inf, -np.inf, np.nan):       # the mask decides alone
        out.append((v, np.full(32, -3.0, dtype=np.float32), f"mask={v}"))
    return out


def edge_planted_at(S, image):
    """Flat pixel indices of the planted pixels in image `image` of a batch: a stride that is no multiple of the wave, shifted per
    image so that the pixels sit in different lanes; every pixel of a 5 x 5 image but two."""
    n, HW = len(edge_planted()), S * S
    step = max(1, (HW - 1) // n)
    step -= 1 if step > 1 and step % 2 == 0 else 0
    return [(k * step + image) % HW for k in range(n)] if step > 1 else [(k + image) % HW for k in range(n)]


def edge_preds(S, image):
    """Image `image` of the edge prediction batch of size S: fp32 [33, S, S], labels -1..3 uniformly at random per pixel."""
    rs = np.random.RandomState(500 + 10 * S + image)
    pos = rs.randint(-1, 4, size=(S, S))
    bits = np.where(pos[None] >= 0, MSGS[np.maximum(pos, 0)].transpose(2, 0, 1), rs.randint(0, 2, size=(32, S, S)))
    out = np.empty((33, S, S), dtype=np.float32)
    out[0] = (4.0 * np.where(pos >= 0, 1.0, -1.0) + 2.0 * rs.randn(S, S)).astype(np.float32)
    out[1:] = (3.0 * (2.0 * bits - 1.0) + 2.5 * rs.randn(32, S, S)).astype(np.float32)
    flat = out.reshape(33, S * S)
    for at, (mask, logits, _) in zip(edge_planted_at(S, image), edge_planted()):
        flat[0, at] = np.float32(mask)
        flat[1:, at] = logits
    return out


def edge_pred_cases():
    """[(S, preds fp32 [3, 33, S, S])]"""
    return [(S, np.stack([edge_preds(S, k) for k in range(3)])) for S in EDGE_POS_SIZES]


# ---- the remove_sync end-to-end test: flat colours per message (tests/sync_standins.py) on a grey image, then index maps
COLOURS = np.array([[0.8, -0.6, -0.6], [-0.6, 0.8, -0.6], [-0.6, -0.6, 0.8], [0.8, 0.8, -0.6]], dtype=np.float32)   # [-1, 1] pixels
E2E = ("untouched", "flip", "rot10", "crop0.7")


def e2e_positions(S=256):
    g = grid_positions(S)
    return np.stack([g, g[:, ::-1], rotate(g, 10, -1), crop_resize(g, 0.7)]).astype(np.int8)


def e2e_images(S=256):
    """[4, 3, S, S] fp32 in [-1, 1]: the synchronised grey image, then the same under a flip, a rotation by 10 degrees and an
    upper-left crop of 0.7 resized back (index maps, so the label map of each is e2e_positions exactly)."""
    pos = e2e_positions(S)
    img = np.zeros((4, 3, S, S), dtype=np.float32)
    for k in range(4):
        for c in range(3):
            img[:, c][pos == k] = COLOURS[k, c]
    return img
