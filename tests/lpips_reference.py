"""LPIPS restated with plain torch ops on a plain state dict in the reference module's key layout
(deps/taming/modules/losses/lpips.py:41-122 in .eval()): the yardstick of the narrow nets and of the per-layer checks.  Runs in the dtype
it is given (float64: the reference; float32: the budget torch's own fp32 arithmetic needs on the same data).

tests/test_lpips_cpu.py holds it to the reference module itself through tests/golden/lpips_vectors.npz."""
import torch
import torch.nn.functional as F

SLICE_CONVS = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))


def features(state, x, dtype):
    """The five taps (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3) of the scaled image."""
    h = (x.to(dtype) - state["scaling_layer.shift"].to(dtype)) / state["scaling_layer.scale"].to(dtype)
    taps = []
    for k, idxs in enumerate(SLICE_CONVS):
        if k > 0:
            h = F.max_pool2d(h, 2, 2)
        for i in idxs:
            p = "net.slice%d.%d." % (k + 1, i)
            h = F.relu(F.conv2d(h, state[p + "weight"].to(dtype), state[p + "bias"].to(dtype), padding=1))
        taps.append(h)
    return taps


def normalize(x, eps=1e-10):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


def head(f0, f1, w):
    """One tap: f0, f1 [B, C, H, W], w [C] (or [1, C, 1, 1]) -> [B]."""
    d = (normalize(f0) - normalize(f1)) ** 2
    return (d * w.reshape(1, -1, 1, 1).to(d.dtype)).sum(1, keepdim=True).mean([2, 3]).reshape(-1)


def lpips(state, inp, target, dtype=torch.float64):
    """-> (value [B], per_tap [5, B]); differentiable towards ``inp``."""
    t0, t1 = features(state, inp, dtype), features(state, target, dtype)
    per_tap = [head(a, b, state["lin%d.model.1.weight" % k]) for k, (a, b) in enumerate(zip(t0, t1))]
    val = per_tap[0]
    for t in per_tap[1:]:
        val = val + t
    return val, torch.stack(per_tap)


def value_and_grad(state, inp, target, dtype=torch.float64, grad_value=None):
    """-> (value [B], per_tap [5, B], d sum_b grad_value[b] value[b] / d inp, all-zero feature vectors of the input branch per tap)."""
    x = inp.detach().to(dtype).requires_grad_(True)
    val, per_tap = lpips(state, x, target.detach(), dtype)
    gv = torch.ones_like(val) if grad_value is None else grad_value.to(dtype)
    (val * gv).sum().backward()
    with torch.no_grad():
        zeros = [int((t.abs().sum(1) == 0).sum()) for t in features(state, inp, dtype)]
    return val.detach(), per_tap.detach(), x.grad, zeros
