"""The fine-tuning step as finetune.py runs it -- decode -> transform -> re-encode, with a frozen original decoder and the L1 (+ LPIPS)
regulariser, differentiated to every encoder and decoder weight -- on the torch stand-in tokenizers (tests/vq_grad_reference.py,
tests/mvq_grad_reference.py, tests/lpips_reference.py), in float64 (the reference) or float32 (the budget torch's own arithmetic needs).
Shared by tests/test_rcc_chain_reference.py (CPU) and tests/test_gpu_rcc_chain.py.

Nothing here restates ``rcc_loss``: `run` calls ``wmar_amd.finetune.rcc_loss`` itself, on the stand-ins or on the device handles.  Three
decisions of the chain are discrete and cannot be left to each dtype; `injected` takes them from the run the reference is compared with
and patches ``Rotate.forward``, ``JPEG.forward`` and ``GaussianNoise.forward`` for the duration of the reference run only.  The classes
stay what they are, so ``apply_random_augmentation``'s ``module_cls is JPEG`` branch and ``idempotence_region``'s ``is Rotate`` /
``is UpperLeftCropWithPadBack`` branches run as shipped:

  Rotate          the whole-operation index map (the forward applied to an image holding 1 .. H W; 0 marks fill), applied as a gather;
  JPEG            the coded image, in [0, 1]; the straight-through form around it is the CPU module's;
  GaussianNoise   the noise tensor.

`margins` reports, from the float64 run, how far the inputs keep every continuous decision from its edge: the smallest distance of a
value in front of a clamp from a clamp bound, and the smallest non-zero |xrec - xrec_orig| (the sign of the L1 term).  The clamps of
the chain, in [0, 1] units with u = 0.5 xrec + 0.5, are those of the three transforms that clamp -- blur(u), u + std noise, factor u --
and MaskGIT's decoder output v in front of ``clamp(v, 0, 1)``.  The identity, Rotate and UpperLeftCropWithPadBack move u and clamp
nothing, and JPEG's clamp of u decides only the coded image, which is injected, while its gradient is the identity
(``apply_random_augmentation`` forms the straight-through sum outside the module): for these four no clamp decision exists between
the decoder and the encoder, so none can differ.  The distance of u itself from 0 and 1 is still reported (``u``), not gated: of
the 98 304 pixels of a 128 x 128 pair some always lie within 1e-5 of a bound that nothing there reads.  MaskGIT saturates about half of
its pixels: there u is exactly 0 or 1, in every dtype and on the device (asserted by the GPU test), and the decoder's clamp passes no
gradient, so a transform value that depends on saturated pixels alone carries nothing to any weight whichever way its clamp falls.
Such values are left out: the transform margin is taken over the output pixels whose footprint holds at least one unsaturated pixel
(the transform's linear part applied to the indicator of those is non-zero)."""
import contextlib
import functools
import random

import torch

from tests import lpips_reference as LR
from tests import mvq_grad_reference as M
from tests import vq_grad_reference as G
from wmar_amd import finetune as ft
from wmar_amd.augmentations.geometric import Rotate, UpperLeftCropWithPadBack
from wmar_amd.augmentations.valuemetric import JPEG, Brightness, GaussianBlur, GaussianNoise, gaussian_blur, jpeg_compress

LOSS_WEIGHT = 2.0
PERCEPTUAL_WEIGHT = 0.5
ORIG_STD, ORIG_SEED = 0.01, 1          # the frozen original decoder: every tensor + 0.01 randn, a generator seeded 1 per tensor
STEP_STD, STEP_SEED = 0.005, 3         # the weight change between the two steps of the second-step cases
NOISE_SEED = 7                         # torch's generators (CPU and device) are seeded with this in front of every chain
MARGIN = 1e-5                          # every clamp margin and the L1 sign margin of the float64 run must reach this
NARROW = (8, 16, 32, 32, 32)
HARNESS128 = dict(ch=32, ch_mult=(1, 2, 2), num_res_blocks=1, attn_resolutions=(8,), resolution=128, z_channels=16, embed_dim=8, n_embed=16384)

CLASSES = {c.__name__: c for c in (JPEG, GaussianBlur, GaussianNoise, Brightness, Rotate, UpperLeftCropWithPadBack)}

# tokenizer -> (state seed, code seed, [(class name, parameter)]); None = no augmentation
TOKENIZERS = {
    "taming": (5, 11, [None] + [("JPEG", q) for q in (90, 20)] + [("GaussianBlur", k) for k in (1, 3, 9)]
               + [("GaussianNoise", s) for s in (0.005, 0.1)] + [("Brightness", f) for f in (1.0, 1.3, 2.0)]
               + [("Rotate", a) for a in (-1, 3, -3)] + [("UpperLeftCropWithPadBack", c) for c in (0.5, 0.7, 0.9)]),
    "lpips": (5, 11, [None, ("Rotate", 3), ("UpperLeftCropWithPadBack", 0.5), ("JPEG", 40)]),
    "maskgit": (5, 12, [None, ("JPEG", 20), ("GaussianBlur", 9), ("GaussianNoise", 0.1), ("Brightness", 2.0), ("Rotate", 3),
                        ("UpperLeftCropWithPadBack", 0.9)]),
    "chameleon": (5, 250, [None, ("GaussianBlur", 9), ("Rotate", -3), ("UpperLeftCropWithPadBack", 0.6), ("JPEG", 20)]),
}
SECOND_STEP = ("taming", "maskgit")     # after Rotate 3 at B = 2: the weights move, then UpperLeftCropWithPadBack 0.5 at B = 1
FIRST, SECOND = ("Rotate", 3), ("UpperLeftCropWithPadBack", 0.5)
ROTATE_REGION = {"taming": slice(1, 7), "lpips": slice(4, 28), "maskgit": slice(1, 7), "chameleon": slice(1, 7)}


def case_id(aug):
    return "none" if aug is None else "%s-%s" % aug


def cases():
    """Every (tokenizer, augmentation, step) the GPU test runs: step 1 at B = 2, step 2 (after the weight change) at B = 1."""
    out = [(name, aug, 1) for name, (_, _, augs) in TOKENIZERS.items() for aug in augs]
    return out + [(name, SECOND, 2) for name in SECOND_STEP]


def resolve(aug):
    return None if aug is None else (CLASSES[aug[0]], aug[1])


# ------------------------------------------------------------------------------------------------ configurations and weights
@functools.lru_cache(maxsize=None)
def config(name):
    import finetune as cli
    from wmar_amd.utils import synth
    if name == "taming":
        return synth.VQConfig(**synth.HARNESS_VQ)
    if name == "lpips":
        return synth.VQConfig(**HARNESS128)
    if name == "chameleon":
        return synth.VQConfig(**cli.CHAMELEON_SMALL_VQ)
    return synth.MaskgitVQConfig(hidden_channels=32, channel_mult=(1, 2, 2), num_res_blocks=1, resolution=32, z_channels=16, num_embeddings=512)


def n_codes(name):
    cfg = config(name)
    return cfg.num_embeddings if name == "maskgit" else cfg.n_embed


def _trainable(key):
    return not key.startswith("quantize.")


@functools.lru_cache(maxsize=None)
def states(name, step=1):
    """(trained state, original state) in fp32 on the CPU: what both sides start from.  Step 2 adds the seeded change to every trainable
    tensor of the trained state, in fp32, as the device side does in place."""
    from wmar_amd.utils import synth
    cfg, seed = config(name), TOKENIZERS[name][0]
    sd = (synth.synth_maskgit_state if name == "maskgit" else synth.synth_vq_state)(cfg, seed, "cpu")
    sd = {k: v.detach().to(torch.float32).contiguous() for k, v in sd.items()}
    orig = {k: (v + ORIG_STD * torch.randn(v.shape, generator=torch.Generator().manual_seed(ORIG_SEED))).to(torch.float32).contiguous()
            for k, v in sd.items()}
    if step == 2:
        sd = {k: v + step_delta(name)[k] if _trainable(k) else v for k, v in sd.items()}
    return sd, orig


@functools.lru_cache(maxsize=None)
def step_delta(name):
    sd, _ = states(name, 1)
    g = torch.Generator().manual_seed(STEP_SEED)
    return {k: STEP_STD * torch.randn(v.shape, generator=g) for k, v in sd.items() if _trainable(k)}


@functools.lru_cache(maxsize=None)
def codes(name, step=1):
    cfg = config(name)
    idx = torch.randint(0, n_codes(name), (2, cfg.codes_size ** 2), generator=torch.Generator().manual_seed(TOKENIZERS[name][1]))
    return idx if step == 1 else idx[:1]


@functools.lru_cache(maxsize=None)
def lpips_state():
    from wmar_amd.utils.synth import synth_lpips_state
    return synth_lpips_state(NARROW, seed=1)


def standins(name, dtype, step=1):
    """(trained stand-in, original stand-in, rec_loss or None) on the CPU in `dtype`."""
    sd, orig = states(name, step)
    T = M.TorchTokenizer if name == "maskgit" else G.TorchTokenizer
    rec = None
    if name == "lpips":
        rec = ft.reference_rec_loss(lambda a, b: LR.lpips(lpips_state(), a, b, dtype)[0], PERCEPTUAL_WEIGHT)
    return T(config(name), sd, dtype), T(config(name), orig, dtype), rec


# ------------------------------------------------------------------------------------------------ the injected decisions
def gather(image, index_map):
    """image [..., H, W] through a whole-operation index map [H, W] holding 0 (fill) or 1 + the flat source position."""
    flat = image.flatten(-2)
    padded = torch.cat([torch.zeros_like(flat[..., :1]), flat], dim=-1)
    return padded[..., index_map.reshape(-1)].view(image.shape)


@contextlib.contextmanager
def injected(decisions):
    """Patches the forwards of the classes `decisions` names: ``rotate_map`` [H, W] int64, ``jpeg_coded`` [B, 3, H, W] in [0, 1],
    ``noise`` [B, 3, H, W].  Restored on exit."""
    decisions = decisions or {}
    saved = []

    def patch(cls, fn):
        saved.append((cls, cls.__dict__["forward"]))
        cls.forward = fn

    if "rotate_map" in decisions:
        patch(Rotate, lambda self, image, angle=None: gather(image, decisions["rotate_map"]))
    if "jpeg_coded" in decisions:
        def jpeg(self, image, quality=None):
            image = image.clamp(0, 1)
            coded = decisions["jpeg_coded"].to(image.device)
            return (image + (coded - image).detach()).clamp(0, 1)
        patch(JPEG, jpeg)
    if "noise" in decisions:
        patch(GaussianNoise, lambda self, image, std=None: (image + std * decisions["noise"].to(image.device, image.dtype)).clamp(0, 1))
    try:
        yield
    finally:
        for cls, fn in saved:
            cls.forward = fn


def index_image(R, dtype=torch.float32):
    return torch.arange(1, R * R + 1, dtype=dtype).view(1, 1, R, R)


def identity_map(R):
    return torch.arange(1, R * R + 1).view(R, R)


def cpu_decisions(tok, idx, aug, dtype):
    """The three decisions as the CPU modules themselves take them in `dtype` for this stand-in and these codes."""
    if aug is None or aug[0] not in (Rotate, JPEG, GaussianNoise):
        return {}
    with torch.no_grad():
        xrec = tok.decode(tok.embed(idx))
        if aug[0] is Rotate:
            R = xrec.shape[-1]
            return {"rotate_map": Rotate()(index_image(R, dtype), aug[1]).round().long().view(R, R)}
        if aug[0] is JPEG:
            u = (0.5 * xrec + 0.5).clamp(0, 1)
            return {"jpeg_coded": torch.stack([jpeg_compress(one, aug[1]) for one in u])}
        torch.manual_seed(NOISE_SEED)
        return {"noise": torch.randn_like(xrec)}


# ------------------------------------------------------------------------------------------------ one step
def run(tok, orig, idx, aug, decisions=None, rec_loss=None):
    """One ``rcc_loss`` step at p = 1 with the one (class, parameter) of `aug` (None: no augmentation) and its backward, on stand-ins or
    on device handles: loss, the log dict, the intermediates, the gradient that lands on xrec (the regulariser's and the
    transform's, summed) and every weight gradient."""
    for p in tok.parameters():
        p.grad = None
    augs = [] if aug is None else [(aug[0], [aug[1]])]
    random.seed(0)
    torch.manual_seed(NOISE_SEED)
    with injected(decisions):
        loss, res, log, was = ft.rcc_loss(tok, idx, augs, p=1.0, loss_weight=LOSS_WEIGHT, orig=orig, rec_loss=rec_loss)
    assert was == (aug is not None)
    res["rec_x"].retain_grad()
    loss.backward()
    out = {"loss": loss.detach(), "log": log, "grads": {k: p.grad.detach().clone() for k, p in tok.named_parameters()},
           "rec_x_grad": res["rec_x"].grad.detach().clone()}
    for k in ("rec_x", "rec_x_maybe_augmented", "rec_z", "rec_x_orig_decoder", "orig_z_q"):
        out[k] = res[k].detach()
    return out


def reference(name, aug, dtype, decisions, step=1):
    """The chain on the stand-ins of `name` in `dtype` under the given decisions; with float64 the margins are added."""
    tok, orig, rec = standins(name, dtype, step)
    out = run(tok, orig, codes(name, step), resolve(aug), decisions, rec)
    if dtype == torch.float64:
        out["margins"] = margins(name, tok, resolve(aug), decisions, out)
    return out


# ------------------------------------------------------------------------------------------------ margins of the float64 run
def margins(name, tok, aug, decisions, out):
    """{"clamp": smallest distance of a relevant value in front of a clamp of the chain from 0 or 1, in [0, 1] units (inf when the chain
    has no clamp), "l1": smallest non-zero |xrec - xrec_orig|, "u": the same distance for u = 0.5 xrec + 0.5 itself (reported only),
    "saturated": MaskGIT's share of pixels at +-1 (0 elsewhere)}; see the module docstring."""
    with torch.no_grad():
        x = out["rec_x"]
        u = 0.5 * x + 0.5
        unsat = torch.ones_like(u, dtype=torch.bool)
        dist = lambda t: torch.minimum(t.abs(), (t - 1.0).abs())      # noqa: E731
        found = [float("inf")]
        if name == "maskgit":
            v = M.decode_preclamp(tok.state, tok.cfg, out["orig_z_q"])
            unsat = (v > 0) & (v < 1)
            found.append(float(dist(v).min()))
        cls, param = aug if aug is not None else (None, None)
        if cls is GaussianBlur:
            found.append(float(dist(gaussian_blur(u, param))[gaussian_blur(unsat.to(u.dtype), param) > 0].min()))
        elif cls is GaussianNoise:
            found.append(float(dist(u + param * decisions["noise"].to(u.dtype))[unsat].min()))
        elif cls is Brightness:
            found.append(float(dist(u * param)[unsat].min()))
        d = (x - out["rec_x_orig_decoder"]).abs()
        return {"clamp": min(found), "l1": float(d[d > 0].min()), "u": float(dist(u)[unsat].min()),
                "saturated": 1.0 - float(unsat.double().mean())}
