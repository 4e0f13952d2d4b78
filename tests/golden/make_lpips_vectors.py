"""Known answers of the reference's LPIPS module (deps/taming/modules/losses/lpips.py) for tests/test_lpips_cpu.py and
tests/test_gpu_lpips.py.  Run once against a checkout of the reference:

    python tests/golden/make_lpips_vectors.py --ref /path/to/reference

The reference file is loaded as it is, behind two fabricated stand-ins for what it imports and this environment lacks (as make_golden.py
does for timm / loguru): a ``torchvision.models.vgg16`` whose ``.features`` is an ``nn.Sequential`` in torchvision's published layer
order (cfg "D": 64, 64, M, 128, 128, M, 256, 256, 256, M, 512, 512, 512, M, 512, 512, 512, M; conv3x3 + ReLU(inplace)), built here, and
a ``deps.taming.util.get_ckpt_path`` that returns nothing; ``load_from_pretrained`` is a no-op (there is no download).  The module then
loads ``synth_lpips_state(seed)`` with ``strict=True`` -- which pins the key layout -- is converted to float64 and run, forward and
autograd, on two seeded image batches at S = 128, B = 2.

Written: lpips_vectors.npz (the two inputs as float32, values and per-tap terms as float64, the count of all-zero feature vectors of the
input branch per tap, a SHA-256 over the weight bytes) and lpips_vectors_grad.npz (the gradient towards ``input`` as float64) -- two
files because each has to stay below the repository's 1 MiB limit for a committed file."""
import argparse
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

SEED, S, B = 0, 128, 2
VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")


def weights_sha256(state) -> str:
    h = hashlib.sha256()
    for k in state:
        h.update(k.encode())
        h.update(state[k].detach().to(torch.float32).contiguous().numpy().tobytes())
    return h.hexdigest()


def make_inputs(seed=SEED, b=B, s=S):
    g = torch.Generator().manual_seed(seed + 77)
    x = torch.rand(b, 3, s, s, generator=g) * 2 - 1
    t = (x + 0.1 * torch.randn(b, 3, s, s, generator=g)).clamp(-1, 1)
    return x, t


def _stand_ins():
    class _Vgg(nn.Module):
        def __init__(self):
            super().__init__()
            layers, cin = [], 3
            for v in VGG16_CFG:
                if v == "M":
                    layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
                else:
                    layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                    cin = v
            self.features = nn.Sequential(*layers)

    tv, models = types.ModuleType("torchvision"), types.ModuleType("torchvision.models")
    models.vgg16 = lambda pretrained=False, **kw: _Vgg()
    tv.models = models
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models
    for name in ("deps", "deps.taming", "deps.taming.util"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["deps.taming.util"].get_ckpt_path = lambda *a, **k: None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    from wmar_amd.utils.synth import synth_lpips_state
    _stand_ins()
    spec = importlib.util.spec_from_file_location("ref_lpips", os.path.join(args.ref, "deps", "taming", "modules", "losses", "lpips.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.LPIPS.load_from_pretrained = lambda self, name="vgg_lpips": None
    state = synth_lpips_state(seed=SEED)
    net = mod.LPIPS().eval()
    net.load_state_dict(state, strict=True)
    net = net.double()
    x, t = make_inputs()
    xi = x.double().requires_grad_(True)
    # the per-tap terms, as forward() builds them
    outs0, outs1 = net.net(net.scaling_layer(xi)), net.net(net.scaling_layer(t.double()))
    lins = [net.lin0, net.lin1, net.lin2, net.lin3, net.lin4]
    per_tap = torch.stack([mod.spatial_average(lins[k].model((mod.normalize_tensor(outs0[k]) - mod.normalize_tensor(outs1[k])) ** 2)).reshape(-1)
                           for k in range(5)])
    zeros = [int((outs0[k].abs().sum(1) == 0).sum()) for k in range(5)]
    val = net(xi, t.double())
    assert val.shape == (B, 1, 1, 1) and torch.allclose(val.reshape(-1), per_tap.sum(0), rtol=1e-13, atol=0)
    val.sum().backward()
    np.savez(os.path.join(HERE, "lpips_vectors.npz"), input=x.numpy(), target=t.numpy(), value=val.detach().reshape(-1).numpy(),
             per_tap=per_tap.detach().numpy(), zero_vectors=np.array(zeros, dtype=np.int64), seed=np.int64(SEED),
             weights_sha256=np.array(weights_sha256(state)))
    np.savez(os.path.join(HERE, "lpips_vectors_grad.npz"), grad_input=xi.grad.numpy())
    print("value", val.detach().reshape(-1).tolist(), "max|grad|", float(xi.grad.abs().max()), "zero vectors", zeros)


if __name__ == "__main__":
    main()
