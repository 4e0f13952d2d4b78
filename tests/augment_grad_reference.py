"""Reference gradients of the device transforms (wmar_augment / wmar_augment_backward, wmar_amd/csrc/augment.hip), in plain torch on
the CPU, float64 unless a dtype is given.  Shared by tests/test_augment_grad_reference.py (CPU) and tests/test_gpu_augment_grad.py.

The forward of the launch is  out = S(clamp(T(R(x))))  with R(x) = x / 2 + 0.5 and S(c) = 2 c - 1 in `pm1` mode (identities otherwise);
the clamp is applied always in `pm1` mode and otherwise only by blur, noise and brightness.  Every transform T is restated with the
torch expressions of wmar_amd/augmentations/{valuemetric,geometric}.py and differentiated by torch autograd, whose clamp passes the
gradient where 0 <= t <= 1, both bounds included.  Rotation is the exception: the kernel differs from grid_sample at .5 ties, and the
backward must follow the forward, so its T is a gather through an INDEX MAP -- the forward applied to an image holding 1 .. H W
(exact in fp32; 0 marks fill) -- and autograd turns that gather into the scatter-add of g through the map."""
import torch
import torch.nn.functional as TF

from wmar_amd.augmentations.geometric import resize_bilinear, rotate_nearest
from wmar_amd.augmentations.valuemetric import gaussian_blur

IDENTITY, BLUR, NOISE, BRIGHTNESS, ROTATE, FLIP_H, CROP_RESIZE, CROP_PAD = range(8)
CLAMPING = (BLUR, NOISE, BRIGHTNESS)        # the transforms that clamp without pm1
TIE = 1e-5                                  # |t - bound| below which fp32 and fp64 may clip differently


def index_image(H, W, dtype=torch.float32):
    return torch.arange(1, H * W + 1, dtype=dtype).view(1, 1, H, W)


def torch_index_map(H, W, quarters, rest):
    """the index map of the torch restatement (Rotate.forward's CPU path): what the CPU tests use; the GPU tests take the kernel's,
    which tests/test_gpu_augment_forward.py holds to a float64 map pixel by pixel"""
    img = index_image(H, W, torch.float64)
    if quarters % 4:
        img = torch.rot90(img, quarters % 4, dims=(-2, -1))
    return rotate_nearest(img, rest).round().long().view(H, W)


def transform(op, u, p0=0.0, p1=0.0, noise=None, index_map=None):
    """T(u) for u [B, C, H, W] in [0, 1], before any clamp"""
    H, W = u.shape[-2:]
    if op == IDENTITY:
        return u * 1.0
    if op == BLUR:
        return gaussian_blur(u, int(p0))
    if op == NOISE:
        return u + p0 * noise.to(u.dtype)
    if op == BRIGHTNESS:
        return u * p0
    if op == FLIP_H:
        return u.flip(-1)
    if op == CROP_RESIZE:
        return resize_bilinear(u[..., :int(p0), :int(p1)], (H, W))
    if op == CROP_PAD:
        return TF.pad(u[..., :int(p0), :int(p1)], (0, W - int(p1), 0, H - int(p0)), mode="constant", value=0.0)
    if op == ROTATE:
        m = index_map.view(-1)
        picked = u.flatten(-2)[..., (m - 1).clamp(min=0)]
        return torch.where(m > 0, picked, torch.zeros((), dtype=u.dtype)).view(u.shape)
    raise ValueError(op)


class Ref:
    """grad: d<out, g>/dx; t: T(R(x)) before the clamp; clamps: whether this call clamps; gm: g where the clamp passes, else 0;
    adjoint_abs(m): the adjoint of T's linear part applied to |m| -- with m = gm the error scale A = sum |w| |g mask| of a pixel"""


def reference(op, x, g, p0=0.0, p1=0.0, noise=None, pm1=False, index_map=None, dtype=torch.float64):
    x = x.detach().to(dtype).clone().requires_grad_(True)
    g = g.detach().to(dtype)
    u = x / 2.0 + 0.5 if pm1 else x
    t = transform(op, u, p0, p1, noise, index_map)
    clamps = bool(pm1) or op in CLAMPING
    c = t.clamp(0, 1) if clamps else t
    out = c * 2.0 - 1.0 if pm1 else c
    out.backward(g)
    r = Ref()
    r.grad, r.t, r.clamps, r.out = x.grad.detach(), t.detach(), clamps, out.detach()
    r.gm = g * ((r.t >= 0) & (r.t <= 1)).to(dtype) if clamps else g

    def adjoint_abs(m):
        z = torch.zeros_like(r.t, requires_grad=True)
        lin = transform(op, z, p0, p1, torch.zeros_like(r.t) if noise is not None else None, index_map)
        lin.backward(m.to(dtype).abs())
        return z.grad.detach()
    r.adjoint_abs = adjoint_abs
    return r


def tie_mask(t64, clamps):
    """output pixels whose float64 t lies within TIE of a clamp bound (all False when the call does not clamp)"""
    if not clamps:
        return torch.zeros_like(t64, dtype=torch.bool)
    return ((t64 - 0.0).abs() < TIE) | ((t64 - 1.0).abs() < TIE)


def zero_ties(op, x, g, **kw):
    """g with the output pixels at a float64 clamp tie set to 0, and the fraction of pixels that were"""
    r = reference(op, x, g, **kw)
    ties = tie_mask(r.t, r.clamps)
    return torch.where(ties, torch.zeros_like(g), g), float(ties.float().mean())


def smallest_c(got, ref):
    """the smallest c with |got - ref.grad| <= c 2^-24 A per pixel, A = the float64 adjoint applied to |g mask|; where A is 0 the two
    must agree exactly (returns inf otherwise)"""
    A = ref.adjoint_abs(ref.gm)
    d = (got.detach().cpu().double() - ref.grad).abs()
    if bool(((A == 0) & (d > 0)).any()):
        return float("inf")
    ratio = torch.where(A > 0, d / (A * 2.0 ** -24), torch.zeros_like(d))
    return float(ratio.max())
