"""CPU: what LPIPS on the device rests on -- the float64 restatement (tests/lpips_reference.py) against the reference module's own
results (tests/golden/lpips_vectors.npz, written by tests/golden/make_lpips_vectors.py), the ABI, the state mapping, the loss and the
flags of the finetune CLI."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import lpips_reference as LR
from tests.conftest import REPO

GOLDEN = os.path.join(REPO, "tests", "golden")
NEW_SYMBOLS = ["wmar_lpips_create", "wmar_lpips_destroy", "wmar_lpips_device_bytes", "wmar_lpips_forward", "wmar_lpips_backward",
               "wmar_lpips_probe_input", "wmar_lpips_probe_input_backward", "wmar_lpips_probe_relu_pool",
               "wmar_lpips_probe_relu_pool_backward", "wmar_lpips_probe_head", "wmar_lpips_probe_head_backward"]


def test_restatement_reproduces_the_reference_module_in_float64():
    from wmar_amd.utils.synth import lpips_shapes, synth_lpips_state
    v = np.load(os.path.join(GOLDEN, "lpips_vectors.npz"))
    g = np.load(os.path.join(GOLDEN, "lpips_vectors_grad.npz"))["grad_input"]
    state = synth_lpips_state(seed=int(v["seed"]))
    assert list(state) == list(lpips_shapes()) and all(tuple(state[k].shape) == s for k, s in lpips_shapes().items())
    h = hashlib.sha256()
    for k in state:
        h.update(k.encode())
        h.update(state[k].numpy().tobytes())
    assert h.hexdigest() == str(v["weights_sha256"]), "synth_lpips_state drifted from the fixture's weights: regenerate the fixture"
    assert v["input"].dtype == np.float32 and v["input"].shape == (2, 3, 128, 128) and g.dtype == np.float64 and g.shape == v["input"].shape
    val, per_tap, grad, zeros = LR.value_and_grad(state, torch.from_numpy(v["input"]), torch.from_numpy(v["target"]), torch.float64)
    assert np.abs(val.numpy() - v["value"]).max() <= 1e-12 * np.abs(v["value"]).max()
    assert np.abs(per_tap.numpy() - v["per_tap"]).max() <= 1e-12 * np.abs(v["per_tap"]).max()
    assert np.abs(grad.numpy() - g).max() <= 1e-12 * np.abs(g).max()
    assert zeros == v["zero_vectors"].tolist()
    assert np.all(v["value"] > 0) and np.abs(g).max() > 0


def test_new_symbols_are_declared_listed_and_exported():
    from wmar_amd import _lib
    header = open(os.path.join(REPO, "include", "wmar_hip.h")).read()
    declared = set(re.findall(r"\b(wmar_[a-z0-9_]+)\s*\(", header))
    L = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SYMBOLS and hasattr(L, s), s
    assert {s for s in declared if s.startswith("wmar_lpips_")} == set(NEW_SYMBOLS)


def test_config_struct_matches_the_compiled_header(tmp_path):
    from wmar_amd import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wmar_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(wmar_lpips_config));']
    for fname, _ in _lib.LpipsConfig._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(wmar_lpips_config, {fname}));')
    lines += ['return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "abi")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "abi")]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(_lib.LpipsConfig) == 28
    for fname, _ in _lib.LpipsConfig._fields_:
        assert int(got[fname]) == getattr(_lib.LpipsConfig, fname).offset


def test_synthetic_state_follows_the_documented_distributions():
    from wmar_amd.utils.synth import synth_lpips_state
    a, b, c = synth_lpips_state(seed=3), synth_lpips_state(seed=3), synth_lpips_state(seed=4)
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["net.slice1.0.weight"], c["net.slice1.0.weight"])
    w = a["net.slice3.12.weight"]
    assert w.shape == (256, 256, 3, 3) and abs(float(w.std()) / (2.0 / (9 * 256)) ** 0.5 - 1) < 0.02
    assert abs(float(a["net.slice4.19.bias"].std()) / 0.05 - 1) < 0.15
    for k in range(5):
        lin = a["lin%d.model.1.weight" % k]
        assert float(lin.min()) >= 0 and float(lin.max()) <= 1.0 / lin.shape[1]
    n = synth_lpips_state((8, 16, 32, 32, 32), seed=0)
    assert n["net.slice1.0.weight"].shape == (8, 3, 3, 3) and n["net.slice2.5.weight"].shape == (16, 8, 3, 3) and n["lin4.model.1.weight"].shape == (1, 32, 1, 1)


def test_from_files_maps_torchvision_and_lin_dicts_onto_the_reference_layout(tmp_path):
    from wmar_amd.lpips import state_from_vgg_and_lin
    from wmar_amd.utils.synth import LPIPS_SCALE, LPIPS_SHIFT, lpips_shapes, synth_lpips_state
    ref = synth_lpips_state(seed=2)
    vgg = {}
    for k, t in ref.items():
        m = re.fullmatch(r"net\.slice\d\.(\d+)\.(weight|bias)", k)
        if m:
            vgg["features.%s.%s" % (m.group(1), m.group(2))] = t
    vgg["classifier.0.weight"] = torch.zeros(4, 4)                              # torchvision's dict holds more than the features
    lin = {k: t for k, t in ref.items() if k.startswith("lin")}
    got = state_from_vgg_and_lin(vgg, lin)
    assert list(got) == list(lpips_shapes())
    assert all(torch.equal(got[k], ref[k]) for k in ref)
    assert got["scaling_layer.shift"].reshape(-1).tolist() == pytest.approx(list(LPIPS_SHIFT)) and got["scaling_layer.scale"].reshape(-1).tolist() == pytest.approx(list(LPIPS_SCALE))
    del vgg["features.28.bias"]
    with pytest.raises(KeyError, match="features.28.bias"):
        state_from_vgg_and_lin(vgg, lin)
    with pytest.raises(KeyError, match="lin3"):
        state_from_vgg_and_lin({**vgg, "features.28.bias": ref["net.slice5.28.bias"]}, {k: v for k, v in lin.items() if not k.startswith("lin3")})


def test_reference_rec_loss_is_the_mean_of_l1_plus_lpips():
    from wmar_amd.finetune import reference_rec_loss

    class Stub:
        def __call__(self, inp, target):
            self.args = (inp, target)
            return ((inp - target) ** 2).mean((1, 2, 3), keepdim=True) * 3.0

    g = torch.Generator().manual_seed(0)
    a = torch.randn(3, 3, 16, 16, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(3, 3, 16, 16, generator=g, dtype=torch.float64)
    for weight in (1.0, 0.25):
        stub = Stub()
        rec = reference_rec_loss(stub, weight)
        got = rec(a, b)
        p = stub(a, b)
        want = torch.mean((a - b).abs() + weight * p)                            # vqperceptual.py:83-92: rec_loss + perceptual_weight * p_loss
        assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want))
        assert stub.args[0] is a, "the gradient goes to LPIPS's first argument: xrec must be handed there"
        assert abs(float(rec.perceptual_component) - float(p.mean())) <= 1e-15
        ga, = torch.autograd.grad(got, a)
        gw, = torch.autograd.grad(want, a)
        assert float((ga - gw).abs().max()) <= 1e-12 * float(gw.abs().max())


def test_rcc_loss_logs_the_perceptual_component_only_when_the_callable_carries_one():
    from wmar_amd import finetune as ft

    class Tok:
        def __init__(self, scale):
            self.w = torch.tensor(scale, requires_grad=True)

        def embed(self, idx):
            return torch.ones(idx.shape[0], 2, 4, 4) * idx.reshape(-1, 1, 4, 4).float()

        def decode(self, z):
            return z.mean(1, keepdim=True).repeat(1, 3, 1, 1) * self.w

        def encode_prequant(self, x):
            return x[:, :2] * self.w

        def quantize(self, z):
            return z, torch.zeros(z.shape[0], 16, dtype=torch.long)

    idx = torch.arange(32).reshape(2, 16)
    rec = ft.reference_rec_loss(lambda a, b: ((a - b) ** 2).mean((1, 2, 3), keepdim=True), 1.0)
    _, _, log, _ = ft.rcc_loss(Tok(1.0), idx, None, orig=Tok(0.5), rec_loss=rec)
    assert log["rec_loss_perceptual_component"] > 0 and log["rec_loss"] > log["rec_loss_perceptual_component"]
    for plain in (None, lambda a, b: (a - b).abs().mean()):
        _, _, log, _ = ft.rcc_loss(Tok(1.0), idx, None, orig=Tok(0.5), rec_loss=plain)
        assert "rec_loss_perceptual_component" not in log and set(log) == {"rec_loss", "idem_loss", "loss", "loss_weight"}


def test_finetune_parser_takes_the_lpips_flags_and_refuses_the_bad_combinations():
    import finetune as cli
    p = cli.build_parser()
    base = "--model taming --synthetic --outdir out "
    a = p.parse_args((base + "--synthetic_config harness128 --synthetic_lpips --perceptual_weight 0.5").split())
    cli.check_args(a)
    assert a.synthetic_lpips and a.perceptual_weight == 0.5 and cli.wants_lpips(a)
    d = p.parse_args(base.split())
    cli.check_args(d)
    assert d.lpips_vgg is None and d.lpips_lin is None and not d.synthetic_lpips and d.perceptual_weight == 1.0 and not cli.wants_lpips(d)
    real = p.parse_args("--model taming --modelpath m --datapath c.pt --lpips_vgg v.pth --lpips_lin l.pth --outdir out".split())
    cli.check_args(real)
    assert cli.wants_lpips(real)
    for bad, msg in (("--model taming --modelpath m --datapath c.pt --lpips_vgg v.pth --outdir out", "go together"),
                     ("--model taming --modelpath m --datapath c.pt --lpips_lin l.pth --outdir out", "go together"),
                     ("--model taming --modelpath m --datapath c.pt --synthetic_lpips --outdir out", "only with --synthetic"),
                     (base + "--synthetic_config harness128 --synthetic_lpips --lpips_vgg v --lpips_lin l", "either"),
                     (base + "--synthetic_config harness --synthetic_lpips", "multiple of 128"),
                     ("--model rar --synthetic --synthetic_config maskgit_small --synthetic_lpips --outdir out", "multiple of 128")):
        with pytest.raises(SystemExit, match=msg):
            cli.check_args(p.parse_args(bad.split()))
    assert cli.load_lpips(d, 32, "cpu") is None
