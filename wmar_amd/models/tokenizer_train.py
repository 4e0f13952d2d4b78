"""Trainable VQGAN tokenizers on the MI355X: ``quant_conv(encoder(x))`` and ``decoder(post_quant_conv(z_q))`` as autograd functions
over the native taped engine (``wmar_vq_train_*``, include/wmar_hip.h; wmar_amd/csrc/vq_train.h).  ``TrainableTokenizer`` is the Taming
network; ``MaskgitTrainableTokenizer`` is RAR's MaskGIT-VQGAN through the same engine and the same class, with another create call.

What the reference trains with ``VQModel.encode`` / ``VQModel.decode`` under torch.autograd (deps/taming/models/vqgan.py:64-73,
86-169; finetune.py).  The parameters ARE the tensors of the wrapper's ``{checkpoint key: tensor}`` state, made leaves with
``requires_grad``: what an optimizer steps is what ``get_image_tokenizer().state_dict()`` returns, and ``on_change`` (the wrapper
drops its packed inference engine) is called whenever a forward finds the weights changed.  The codebook is frozen.

The two forwards are ``torch.autograd.Function``s.  Their backward returns the input gradient and ADDS the weight gradients into the
parameters' ``.grad`` itself (the engine hands over all gradients of a half in one call).  Each half has one tape: a backward must
belong to the LAST forward of its half, anything else raises.  Under ``torch.no_grad()``, or when nothing requires a gradient, the
forwards run on a second engine (created on first use) and leave the tapes alone.  That engine is a forward-only handle
(``wmar_vq_train_create_frozen``): the same executor over the plan's slot buffers, bit-equal outputs, none of the tape or of the
backward's memory.  ``frozen=True`` makes a tokenizer of that handle alone -- the original decoder of the fine-tuning loss: it leaves
``requires_grad`` of its state as it finds it, never builds a taped engine and returns tensors without a graph.  There is no PyTorch
fallback.

The MaskGIT flavour is what the reference's RAR fine-tuning differentiates (deps/rar/modeling/titok.py:91-208): ``decode`` is
``decode_like_taming`` -- ``clamp(decoder(z_q), 0, 1) * 2 - 1``, images in [-1, 1] -- and ``encode_prequant`` is
``encoder((x + 1) / 2)``; the range changes and the clamp are inside the engine's forward and backward.  There is no ``quant_conv`` /
``post_quant_conv`` (``embed_dim == z_channels``), and the block convolutions and ``encoder.conv_in`` have no bias."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Iterator, Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .engine import _require_cuda

_PREFIXES = (("encoder.", 0), ("quant_conv.", 0), ("post_quant_conv.", 1), ("decoder.", 1))


def _half_of(key: str) -> Optional[int]:
    for p, h in _PREFIXES:
        if key.startswith(p):
            return h
    return None


def _vq_config(cfg, max_batch: int) -> "_lib.VqConfig":
    c = _lib.VqConfig()
    c.ch, c.num_res_blocks, c.resolution = cfg.ch, cfg.num_res_blocks, cfg.resolution
    c.in_channels, c.out_ch, c.z_channels = cfg.in_channels, cfg.out_ch, cfg.z_channels
    c.embed_dim, c.n_embed, c.n_levels = cfg.embed_dim, cfg.n_embed, len(cfg.ch_mult)
    for i, m in enumerate(cfg.ch_mult):
        c.ch_mult[i] = m
    c.n_attn_res = len(cfg.attn_resolutions)
    for i, r in enumerate(cfg.attn_resolutions):
        c.attn_resolutions[i] = r
    c.max_batch = int(max_batch)
    return c


def _mvq_config(cfg, max_batch: int) -> "_lib.MvqConfig":
    c = _lib.MvqConfig()
    c.hidden_channels, c.num_res_blocks, c.resolution = cfg.hidden_channels, cfg.num_res_blocks, cfg.resolution
    c.num_channels, c.z_channels, c.num_embeddings = cfg.num_channels, cfg.z_channels, cfg.num_embeddings
    c.n_levels = len(cfg.channel_mult)
    for i, m in enumerate(cfg.channel_mult):
        c.channel_mult[i] = m
    c.max_batch = int(max_batch)
    return c


class _TrainEngine:
    """Owner of one wmar_vq_train handle; ``create`` names the entry that builds it, ``abi_cfg`` is that entry's config struct."""

    def __init__(self, create: str, abi_cfg, tensors: Dict[str, torch.Tensor], device):
        self._L = _lib.load()
        self.device = device
        names, ptrs, n = _lib.tensor_table(tensors)
        h = C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(getattr(self._L, create)(C.byref(abi_cfg), names, ptrs, n, _lib.stream_ptr(device), C.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.wmar_vq_train_destroy(h)
            self._h = None

    @property
    def device_bytes(self) -> int:
        return int(self._L.wmar_vq_train_device_bytes(self._h))

    def call(self, name: str, *args):
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._L, "wmar_vq_train_" + name)(self._h, *args, _lib.stream_ptr(self.device)))


class _Encode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tok, images, *params):
        ctx.tok, ctx.tape = tok, tok._forward(0, images)
        return tok._last_out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gi = ctx.tok._backward(0, ctx.tape, g.permute(0, 2, 3, 1), ctx.needs_input_grad[1])
        return (None, gi) + (None,) * (len(ctx.needs_input_grad) - 2)


class _Decode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tok, z_q, *params):
        ctx.tok, ctx.tape = tok, tok._forward(1, z_q)
        return tok._last_out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gz = ctx.tok._backward(1, ctx.tape, g, ctx.needs_input_grad[1])
        return (None, gz) + (None,) * (len(ctx.needs_input_grad) - 2)


class TrainableTokenizer:
    # what a flavour of the network supplies: the create entry, its config struct, and (code width, image channels in, out)
    _create = "wmar_vq_train_create"
    _abi_config = staticmethod(_vq_config)

    @staticmethod
    def _dims(cfg) -> Tuple[int, int, int]:
        return cfg.embed_dim, cfg.in_channels, cfg.out_ch

    def _engine(self, frozen: bool = False) -> _TrainEngine:
        return _TrainEngine(self._create + ("_frozen" if frozen else ""), self._abi_config(self.cfg, self.max_batch), self._tensors(), self.device)

    def __init__(self, cfg, state: Dict[str, torch.Tensor], max_batch: int = 4, device="cuda", on_change: Optional[Callable[[], None]] = None,
                 frozen: bool = False):
        self.cfg, self.state, self.max_batch = cfg, state, int(max_batch)
        self._E, self._Cin, self._Cout = self._dims(cfg)
        self.device = torch.device(device)
        self._on_change = on_change
        self._keys = [k for k in state if _half_of(k) is not None]
        for k in self._keys:
            t = state[k]
            _require_cuda(t, k)
            if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_leaf:
                raise ValueError(f"TrainableTokenizer: {k} must be a contiguous float32 leaf tensor")
            if not frozen:
                t.requires_grad_(True)
        self.frozen = bool(frozen)
        self._train = None if frozen else self._engine()
        self._eval: Optional[_TrainEngine] = self._engine(frozen=True) if frozen else None
        self._versions = self._current_versions()
        self._tape = [0, 0]            # serial number of the forward each half's tape belongs to
        self._last_out = None

    # ------------------------------------------------------------------ parameters
    def _tensors(self) -> Dict[str, torch.Tensor]:
        return {k: self.state[k].detach() for k in self._keys}

    def _current_versions(self):
        return [self.state[k]._version for k in self._keys]

    def named_parameters(self, prefix: Optional[str] = None) -> Iterator[Tuple[str, torch.Tensor]]:
        """The state tensors as leaves, in checkpoint order; ``prefix`` (a string or a tuple of strings) selects by key prefix."""
        for k in self._keys:
            if prefix is None or k.startswith(prefix):
                yield k, self.state[k]

    def parameters(self, prefix: Optional[str] = None) -> Iterator[torch.Tensor]:
        for _, p in self.named_parameters(prefix):
            yield p

    @property
    def device_bytes(self) -> int:
        return sum(e.device_bytes for e in (self._train, self._eval) if e is not None)

    def _sync_weights(self):
        """Repack (wmar_vq_train_set_weights) when any parameter changed in place since the last pack: optimizer.step() needs no call."""
        now = self._current_versions()
        if now == self._versions:
            return
        names, ptrs, n = _lib.tensor_table(self._tensors())
        if self._train is not None:
            self._train.call("set_weights", names, ptrs, n)
        if self._eval is not None:
            self._eval.call("set_weights", names, ptrs, n)
        self._versions = now
        self._tape = [0, 0]
        if self._on_change is not None:
            self._on_change()

    # ------------------------------------------------------------------ forwards / backwards
    def _run(self, engine: _TrainEngine, half: int, x: torch.Tensor) -> torch.Tensor:
        S, R, B = self.cfg.codes_size, self.cfg.resolution, x.shape[0]
        if half == 0:
            out = torch.empty(B, S, S, self._E, dtype=torch.float32, device=self.device)
            engine.call("encode", x.data_ptr(), B, out.data_ptr())
            return out.permute(0, 3, 1, 2)
        out = torch.empty(B, self._Cout, R, R, dtype=torch.float32, device=self.device)
        engine.call("decode", x.data_ptr(), B, out.data_ptr())
        return out

    def _prepare(self, half: int, x: torch.Tensor) -> torch.Tensor:
        S, R = self.cfg.codes_size, self.cfg.resolution
        want = (self._Cin, R, R) if half == 0 else (self._E, S, S)
        _require_cuda(x, "images" if half == 0 else "z_q")
        if x.ndim != 4 or tuple(x.shape[1:]) != want:
            raise ValueError(f"expected [B, {want[0]}, {want[1]}, {want[2]}], got {tuple(x.shape)}")
        if x.shape[0] < 1 or x.shape[0] > self.max_batch:
            raise ValueError(f"batch {x.shape[0]} outside 1..max_batch={self.max_batch}: a tape holds one chunk, batches are not split")
        x = x.detach().to(torch.float32)
        return x.contiguous() if half == 0 else x.permute(0, 2, 3, 1).contiguous()      # z_q crosses the ABI as [B*S*S, E]

    def _forward(self, half: int, x: torch.Tensor) -> int:
        self._last_out = self._run(self._train, half, self._prepare(half, x))
        self._serial = getattr(self, "_serial", 0) + 1
        self._tape[half] = self._serial
        return self._serial

    def _backward(self, half: int, tape: int, g: torch.Tensor, want_input: bool):
        if self._tape[half] != tape or self._current_versions() != self._versions:
            raise RuntimeError("TrainableTokenizer: this backward does not belong to the last forward of its half (a later forward or a "
                               "weight change replaced the tape)")
        S, R, B = self.cfg.codes_size, self.cfg.resolution, g.shape[0]
        g = g.to(torch.float32).contiguous()
        if half == 0:
            gi = torch.empty(B, self._Cin, R, R, dtype=torch.float32, device=self.device) if want_input else None
            self._train.call("encode_backward", g.data_ptr(), B, gi.data_ptr() if want_input else None)
        else:
            gi = torch.empty(B, S, S, self._E, dtype=torch.float32, device=self.device) if want_input else None
            self._train.call("decode_backward", g.data_ptr(), B, gi.data_ptr() if want_input else None)
            gi = gi.permute(0, 3, 1, 2) if want_input else None
        keys = [k for k in self._keys if _half_of(k) == half and self.state[k].requires_grad]
        for k in keys:
            if self.state[k].grad is None:
                self.state[k].grad = torch.zeros_like(self.state[k])
        if keys:
            names = (C.c_char_p * len(keys))(*[k.encode() for k in keys])
            ptrs = (C.c_void_p * len(keys))(*[self.state[k].grad.data_ptr() for k in keys])
            self._train.call("get_grads", names, ptrs, len(keys), 1)
        return gi

    def _apply(self, fn, half: int, x: torch.Tensor) -> torch.Tensor:
        self._sync_weights()
        params = [p for k, p in self.named_parameters() if _half_of(k) == half and p.requires_grad]
        if not self.frozen and torch.is_grad_enabled() and (x.requires_grad or params):
            return fn.apply(self, x, *params)
        if self._eval is None:
            self._eval = self._engine(frozen=True)
        return self._run(self._eval, half, self._prepare(half, x))

    def encode_prequant(self, images: torch.Tensor) -> torch.Tensor:
        """images [B, 3, R, R] -> quant_conv(encoder(images)) [B, E, S, S] (VQModel.encode before the quantizer)."""
        return self._apply(_Encode, 0, images)

    def decode(self, z_q: torch.Tensor) -> torch.Tensor:
        """z_q [B, E, S, S] -> decoder(post_quant_conv(z_q)) [B, 3, R, R], not clamped (VQModel.decode)."""
        return self._apply(_Decode, 1, z_q)

    # ------------------------------------------------------------------ the frozen quantizer
    @torch.no_grad()
    def embed(self, indices: torch.Tensor) -> torch.Tensor:
        """codes [B, S*S] -> z_q [B, E, S, S] (quantize.embedding, vqgan.py:94-99); no gradient: the codebook is frozen."""
        S = self.cfg.codes_size
        z = self.state["quantize.embedding.weight"].detach()[indices.to(self.device).reshape(-1, S * S)]
        return z.view(-1, S, S, self._E).permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def quantize(self, z: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """z [B, E, S, S] -> (z_q [B, E, S, S], indices [B, S*S]): the engine's nearest-code search (first minimum of |z|^2 + |e|^2 - 2 z.e,
        quantize.py:277-285) on the rows of z; no gradient."""
        S, E = self.cfg.codes_size, self._E
        rows = z.detach().to(torch.float32).permute(0, 2, 3, 1).reshape(-1, E).contiguous()
        emb = self.state["quantize.embedding.weight"].detach().contiguous()
        codes = torch.empty(rows.shape[0], dtype=torch.int64, device=self.device)
        buf = C.create_string_buffer(128)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().wmar_vq_probe_argmin(rows.data_ptr(), rows.shape[0], E, emb.data_ptr(), emb.shape[0], codes.data_ptr(), buf, 128,
                                                        _lib.stream_ptr(self.device)))
        codes = codes.view(-1, S * S)
        return self.embed(codes), codes


class MaskgitTrainableTokenizer(TrainableTokenizer):
    """RAR's MaskGIT-VQGAN (``MaskgitVQConfig``): parameters under ``encoder.`` and ``decoder.`` only.  ``encode_prequant`` takes
    [-1, 1] images to ``encoder((x + 1) / 2)`` [B, z_channels, S, S]; ``decode`` takes z_q to ``clamp(decoder(z_q), 0, 1) * 2 - 1``
    (titok.py:91-123)."""

    _create = "wmar_mvq_train_create"
    _abi_config = staticmethod(_mvq_config)

    @staticmethod
    def _dims(cfg) -> Tuple[int, int, int]:
        return cfg.z_channels, cfg.num_channels, cfg.num_channels
