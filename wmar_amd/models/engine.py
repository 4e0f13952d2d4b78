"""Python handles on the native engines of libwmar_hip.so (GPT decode loop, VQGAN)."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np
import torch

from .. import _lib
from ..utils.synth import GPTConfig, VQConfig


def _require_cuda(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"wmar_amd: {what} must live on the MI355X (no CPU implementation)")


class _Engine:
    """Owner of one native engine handle: `<prefix>_create` / `_destroy` / `_device_bytes` of libwmar_hip.so."""

    _prefix = ""  # "wmar_gpt", ...

    def _create(self, config, state: Dict[str, torch.Tensor], keep, device, max_batch: int, dtype=torch.float32, options=None):
        """Creates the engine from the entries of `state` whose name `keep` accepts, moved to `device` as contiguous `dtype`
        (the engine repacks them into its own HBM buffers: the copies made here are dropped on return).  `options`: the bit set of
        `<prefix>_create_opt` instead of `<prefix>_create`."""
        self.device = torch.device(device)
        self.max_batch = int(max_batch)
        self._L = _lib.load()
        tensors = {k: v.detach().to(device=self.device, dtype=dtype).contiguous() for k, v in state.items() if keep(k)}
        names, ptrs, n = _lib.tensor_table(tensors)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            if options is None:
                rc = getattr(self._L, self._prefix + "_create")(C.byref(config), names, ptrs, n, _lib.stream_ptr(self.device), C.byref(h))
            else:
                rc = getattr(self._L, self._prefix + "_create_opt")(C.byref(config), int(options), names, ptrs, n,
                                                                    _lib.stream_ptr(self.device), C.byref(h))
            _lib.check(rc)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            getattr(self._L, self._prefix + "_destroy")(h)
            self._h = None

    @property
    def device_bytes(self) -> int:
        return int(getattr(self._L, self._prefix + "_device_bytes")(self._h))


class _GraphCounts:
    """The decode engines: how many graph slots the fused and the hooked loop have captured since the engine was created."""

    def graph_counts(self) -> Dict[str, int]:
        """{"fused": n, "hooked": n}; a call that reuses the graphs of an earlier call leaves both unchanged."""
        a, b = C.c_int64(), C.c_int64()
        _lib.check(getattr(self._L, self._prefix + "_graph_counts")(self._h, C.byref(a), C.byref(b)))
        return {"fused": int(a.value), "hooked": int(b.value)}


class _LogitsHook:
    """The host side of a hooked generation (include/wmar_hip.h, "hooked generation"): owns the two buffers the engine and the
    processor share and wraps the processor as the library's C callback.

    ``logits``: float32 [B, V], contiguous; ``past``: int64 [B, width], of which the first ``t`` columns are valid at a step.  The
    processor is called under ``torch.no_grad()`` on the device's current stream (the stream the engine replays its graphs on), as
    ``f(past_ids=past[:, :t], logits=logits)`` or, with ``positional``, ``f(past[:, :t], logits)``.  It returns a [B, V] tensor; if
    that is not the buffer itself it is copied in (``copy_`` converts the dtype).  ctypes swallows what a callback raises, so the
    exception is kept here, the library is told to stop (non-zero return) and ``finish`` re-raises it."""

    def __init__(self, processor, B: int, V: int, width: int, device, positional: bool):
        self.processor, self.positional = processor, positional
        self.logits = torch.empty(B, V, dtype=torch.float32, device=device)
        self.past = torch.zeros(B, width, dtype=torch.int64, device=device)
        self.error = None
        self.cfunc = _lib.LOGITS_HOOK(self._call)

    def _call(self, user, step, t):
        try:
            with torch.no_grad():
                past = self.past[:, :t]
                out = self.processor(past, self.logits) if self.positional else self.processor(past_ids=past, logits=self.logits)
                if not isinstance(out, torch.Tensor):
                    raise TypeError(f"logit processor returned {type(out).__name__}, expected a tensor of shape {tuple(self.logits.shape)}")
                if out.shape != self.logits.shape:
                    raise ValueError(f"logit processor returned shape {tuple(out.shape)}, expected {tuple(self.logits.shape)}")
                if out is not self.logits and not (out.data_ptr() == self.logits.data_ptr() and out.dtype == self.logits.dtype
                                                   and out.is_contiguous()):
                    self.logits.copy_(out)
            return 0
        except BaseException as e:  # noqa: BLE001  (re-raised by finish(): nothing may cross the C frames)
            self.error = e
            return 1

    def finish(self, rc: int):
        """Status of the library call -> the processor's own exception, unchanged, or the library's error."""
        err, self.error = self.error, None
        if err is not None:
            raise err
        _lib.check(rc)


class _TokenizerEngine(_Engine):
    """Chunked (max_batch images per call) encode / decode of the two VQ tokenizers."""

    _out_channels = 0  # image channels of decode()
    _code_dim = 0      # width of the pre-quantization rows encode() can return

    def decode(self, codes: torch.Tensor) -> torch.Tensor:
        _require_cuda(codes, "codes")
        codes = codes.to(torch.int64).contiguous()
        B = codes.shape[0]
        R = self.cfg.resolution
        out = torch.empty(B, self._out_channels, R, R, dtype=torch.float32, device=self.device)
        decode = getattr(self._L, self._prefix + "_decode")
        with torch.cuda.device(self.device):
            for b0 in range(0, B, self.max_batch):
                b1 = min(B, b0 + self.max_batch)
                _lib.check(decode(self._h, codes[b0:b1].data_ptr(), b1 - b0, out[b0:b1].data_ptr(), _lib.stream_ptr(self.device)))
        return out

    def encode(self, images: torch.Tensor, return_prequant: bool = False):
        _require_cuda(images, "images")
        images = images.to(torch.float32).contiguous()
        B = images.shape[0]
        S = self.cfg.codes_size
        codes = torch.empty(B, S * S, dtype=torch.int64, device=self.device)
        pre = torch.empty(B * S * S, self._code_dim, dtype=torch.float32, device=self.device) if return_prequant else None
        encode = getattr(self._L, self._prefix + "_encode")
        with torch.cuda.device(self.device):
            for b0 in range(0, B, self.max_batch):
                b1 = min(B, b0 + self.max_batch)
                _lib.check(encode(self._h, images[b0:b1].data_ptr(), b1 - b0, codes[b0:b1].data_ptr(),
                                  pre[b0 * S * S:b1 * S * S].data_ptr() if pre is not None else None, _lib.stream_ptr(self.device)))
        return (codes, pre) if return_prequant else codes


class GPTEngine(_Engine, _GraphCounts):
    """minGPT with a static KV cache; replaces GPT.forward_with_past + sample_with_past
    (deps/taming/modules/transformer/mingpt.py:183-214, 326-368)."""

    _prefix = "wmar_gpt"
    DEFAULT_FC2X = True     # the measured A/B decides this

    def __init__(self, cfg: GPTConfig, state: Dict[str, torch.Tensor], max_batch: int = 64, device="cuda", fc2x: Optional[bool] = None):
        """fc2x: ask for the two-slab FC2 / QKV seam at 33..64 rows (WMAR_GPT_OPT_FC2X, include/wmar_hip.h; the library applies it
        only where the shape is eligible).  None: DEFAULT_FC2X, unless WMAR_NO_FC2X is set in the environment (A/B runs) or
        max_batch <= 32 (the second packing of mlp.2.weight would never be read)."""
        self.cfg = cfg
        if fc2x is None:
            fc2x = self.DEFAULT_FC2X and not os.environ.get("WMAR_NO_FC2X") and int(max_batch) > 32
        self.fc2x = bool(fc2x)
        c = _lib.GptConfig(cfg.vocab_size, cfg.block_size, cfg.n_layer, cfg.n_head, cfg.n_embd, int(max_batch))
        self._create(c, state, lambda k: not k.endswith("attn.mask"), device, max_batch,
                     options=_lib.GPT_OPT_FC2X if self.fc2x else 0)

    def decode_step(self, tok: torch.Tensor, pos: int) -> torch.Tensor:
        """One token per sequence at position `pos` -> logits [B, V]."""
        _require_cuda(tok, "tokens")
        tok = tok.to(torch.int64).contiguous().view(-1)
        B = tok.shape[0]
        logits = torch.empty(B, self.cfg.vocab_size, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.wmar_gpt_decode_step(self._h, tok.data_ptr(), B, int(pos), logits.data_ptr(),
                                                    _lib.stream_ptr(self.device)))
        return logits

    def _staging(self, cond: torch.Tensor, steps: int, q: torch.Tensor, temperature, top_k, top_p, use_graph: bool):
        """Arguments both generate calls share: cond int64 [B], B, V, the token buffer [B, steps] and the sampling parameters."""
        _require_cuda(cond, "conditioning")
        _require_cuda(q, "q")
        cond = cond.to(torch.int64).contiguous().view(-1)
        B = cond.shape[0]
        V = self.cfg.vocab_size
        assert q.shape == (steps, B, V) and q.dtype == torch.float32 and q.is_contiguous()
        out = torch.empty(B, steps, dtype=torch.int64, device=self.device)
        sp = _lib.SampleParams(float(temperature), int(top_k) if top_k else 0,
                               float(top_p) if top_p is not None else -1.0, 1 if use_graph else 0)
        return cond, B, V, out, sp

    def generate(self, cond: torch.Tensor, steps: int, q: torch.Tensor, temperature=1.0, top_k=None, top_p=None,
                 wm_ctx: Optional[_lib.WmCtx] = None, use_graph: bool = True, trace_logits: bool = False):
        """sample_with_past: cond int64 [B], q float32 [steps, B, V] -> tokens int64 [B, steps]."""
        cond, B, V, out, sp = self._staging(cond, steps, q, temperature, top_k, top_p, use_graph)
        trace = torch.empty(steps, B, V, dtype=torch.float32, device=self.device) if trace_logits else None
        with torch.cuda.device(self.device):
            _lib.check(self._L.wmar_gpt_generate(
                self._h, C.byref(wm_ctx) if wm_ctx is not None else None, C.byref(sp), cond.data_ptr(), B, int(steps),
                q.data_ptr(), out.data_ptr(), trace.data_ptr() if trace is not None else None,
                _lib.stream_ptr(self.device)))
            # waits for the replays; raises if the fused projection launch's in-kernel barrier gave up (results invalid)
            _lib.check(self._L.wmar_gpt_check(self._h, _lib.stream_ptr(self.device)))
        return (out, trace) if trace_logits else out

    def generate_hooked(self, cond: torch.Tensor, steps: int, q: torch.Tensor, processor, temperature=1.0, top_k=None, top_p=None,
                        use_graph: bool = True) -> torch.Tensor:
        """``generate`` with a reference-style ``logit_processor`` between the model step and the sampler (mingpt.py:348-350):
        ``processor(past_ids=int64 [B, n+1] (class token, then the n tokens so far), logits=float32 [B, V] raw head output)``."""
        cond, B, V, out, sp = self._staging(cond, steps, q, temperature, top_k, top_p, use_graph)
        with torch.cuda.device(self.device):
            hook = _LogitsHook(processor, B, V, steps + 1, self.device, positional=False)
            hook.finish(self._L.wmar_gpt_generate_hooked(
                self._h, C.byref(sp), cond.data_ptr(), B, int(steps), q.data_ptr(), out.data_ptr(), hook.logits.data_ptr(),
                hook.past.data_ptr(), hook.past.stride(0), hook.cfunc, None, _lib.stream_ptr(self.device)))
            _lib.check(self._L.wmar_gpt_check(self._h, _lib.stream_ptr(self.device)))
        return out

    def profile_role(self, role: str, B: int, kv_len: int = 128, iters: int = 96) -> float:
        """Average microseconds per launch of one role's kernel replayed back to back (HIP events)."""
        out = C.c_double()
        with torch.cuda.device(self.device):
            _lib.check(self._L.wmar_gpt_profile_role(self._h, self.T_CLASSES.index(role), B, kv_len, iters,
                                                     _lib.stream_ptr(self.device), C.byref(out)))
        return out.value

    def plan_info(self, B: int) -> Dict[str, str]:
        """{role: kernel} of a decode step at batch B, as the engine selects them."""
        buf = C.create_string_buffer(2048)
        _lib.check(self._L.wmar_gpt_plan_info(self._h, int(B), buf, len(buf)))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";"))

    def set_attention_phases(self, one_wave_upto: int, two_waves_upto: int):
        """Cache lengths up to which the decode attention runs 1 / 2 waves per (sequence, head) (4 beyond)."""
        _lib.check(self._L.wmar_gpt_set_attention_phases(self._h, int(one_wave_upto), int(two_waves_upto)))

    def set_timing(self, on: bool):
        self._L.wmar_gpt_set_timing(self._h, 1 if on else 0)

    T_CLASSES = ["embed", "qkv", "attn", "proj", "resid", "fc1", "fc2", "head", "sample"]

    def get_timing(self):
        """{class: (total_us, calls)} of the last eager generate() with timing on, and ms/step."""
        n = len(self.T_CLASSES)
        us = (C.c_double * n)()
        calls = (C.c_int64 * n)()
        step = C.c_double()
        self._L.wmar_gpt_get_timing(self._h, us, calls, C.byref(step))
        return {k: (us[i], calls[i]) for i, k in enumerate(self.T_CLASSES)}, step.value


class VQGANEngine(_TokenizerEngine):
    """Taming VQGAN encode / decode; replaces VQModel.encode/decode + VectorQuantizer2
    (deps/taming/models/vqgan.py:64-73, modules/vqvae/quantize.py:272-331)."""

    _prefix = "wmar_vq"

    def __init__(self, cfg: VQConfig, state: Dict[str, torch.Tensor], max_batch: int = 64, device="cuda"):
        self.cfg = cfg
        self._out_channels, self._code_dim = cfg.out_ch, cfg.embed_dim
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
        self._create(c, state, lambda k: not k.startswith("loss."), device, max_batch)


class RAREngine(_Engine, _GraphCounts):
    """RAR generator with KV cache, adaLN, qk-norm and classifier-free guidance; replaces
    RAR.forward_fn / RAR.generate (deps/rar/modeling/rar.py:319-459)."""

    _prefix = "wmar_rar"

    def __init__(self, cfg, state: Dict[str, torch.Tensor], max_batch: int = 64, device="cuda"):
        self.cfg = cfg
        c = _lib.RarConfig(cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.intermediate_size,
                           cfg.image_seq_len, cfg.codebook_size, cfg.condition_num_classes, int(max_batch))
        self._create(c, state, lambda k: k != "attn_mask", device, max_batch)

    def _staging(self, class_ids: torch.Tensor, cfg_scales: Optional[torch.Tensor]):
        """Arguments both generate calls share: class ids [B], the token buffer [B, L] and the guidance scales as
        (host tensor kept alive, float pointer or None, use_guidance)."""
        _require_cuda(class_ids, "class ids")
        class_ids = class_ids.to(torch.int64).contiguous().view(-1)
        out = torch.empty(class_ids.shape[0], self.cfg.image_seq_len, dtype=torch.int64, device=self.device)
        if cfg_scales is None:
            return class_ids, out, (None, None, 0)
        sc = cfg_scales.detach().to("cpu", torch.float32).contiguous()
        assert sc.numel() == self.cfg.image_seq_len
        return class_ids, out, (sc, C.cast(sc.data_ptr(), C.POINTER(C.c_float)), 1)

    def launch_status(self) -> Dict[str, int]:
        """{"fused": the fused residual + modulation launch is in use, "fallbacks": calls re-run on the two-launch pair}."""
        a, b = C.c_int32(), C.c_int32()
        _lib.check(self._L.wmar_rar_launch_status(self._h, C.byref(a), C.byref(b)))
        return {"fused": int(a.value), "fallbacks": int(b.value)}

    def forward_position(self, tok: torch.Tensor, cond_ids: torch.Tensor, pos: int) -> torch.Tensor:
        """tok int64 [M] (-1 = cls), cond_ids int64 [M] (offset condition ids) -> logits [M, V]."""
        _require_cuda(tok, "tokens")
        tok = tok.to(torch.int64).contiguous().view(-1)
        cond_ids = cond_ids.to(device=self.device, dtype=torch.int64).contiguous().view(-1)
        M = tok.shape[0]
        logits = torch.empty(M, self.cfg.codebook_size, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.wmar_rar_forward_position(self._h, tok.data_ptr(), cond_ids.data_ptr(), M, int(pos),
                                                         logits.data_ptr(), _lib.stream_ptr(self.device)))
        return logits

    def generate(self, class_ids: torch.Tensor, q: torch.Tensor, cfg_scales: Optional[torch.Tensor], temperature=1.0,
                 wm_ctx: Optional[_lib.WmCtx] = None, use_graph: bool = True) -> torch.Tensor:
        """class_ids int64 [B]; q float32 [L, B, V]; cfg_scales float32 [L] on the host (None: no guidance)."""
        class_ids, out, (sc, sc_ptr, guided) = self._staging(class_ids, cfg_scales)
        _require_cuda(q, "q")
        B = class_ids.shape[0]
        assert q.shape == (self.cfg.image_seq_len, B, self.cfg.codebook_size) and q.dtype == torch.float32 and q.is_contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self._L.wmar_rar_generate(
                self._h, C.byref(wm_ctx) if wm_ctx is not None else None, class_ids.data_ptr(), B, sc_ptr, guided,
                float(temperature), q.data_ptr(), out.data_ptr(), 1 if use_graph else 0, _lib.stream_ptr(self.device)))
            _lib.check(self._L.wmar_rar_check(self._h, _lib.stream_ptr(self.device)))      # waits; raises if an in-launch wait gave up
        return out

    def generate_hooked(self, class_ids: torch.Tensor, q: torch.Tensor, cfg_scales: Optional[torch.Tensor], processor,
                        temperature=1.0, use_graph: bool = True) -> torch.Tensor:
        """``generate`` with a reference-style ``logit_processor`` behind the guidance mix (rar.py:437-451):
        ``processor(past_ids=int64 [B, n] (generated tokens only, [B, 0] at the first step), logits=float32 [B, V])``."""
        class_ids, out, (sc, sc_ptr, guided) = self._staging(class_ids, cfg_scales)
        _require_cuda(q, "q")
        B = class_ids.shape[0]
        L, V = self.cfg.image_seq_len, self.cfg.codebook_size
        assert q.shape == (L, B, V) and q.dtype == torch.float32 and q.is_contiguous()
        with torch.cuda.device(self.device):
            hook = _LogitsHook(processor, B, V, L, self.device, positional=False)
            hook.finish(self._L.wmar_rar_generate_hooked(
                self._h, class_ids.data_ptr(), B, sc_ptr, guided, float(temperature), q.data_ptr(), out.data_ptr(),
                1 if use_graph else 0, hook.logits.data_ptr(), hook.past.data_ptr(), hook.past.stride(0), hook.cfunc, None,
                _lib.stream_ptr(self.device)))
            _lib.check(self._L.wmar_rar_check(self._h, _lib.stream_ptr(self.device)))
        return out

    def generate_gumbel(self, class_ids, log_rs, cfg_scales, temperature=1.0, top_p=0.0, top_k=0, use_graph=True):
        """RAR.generate with the Gumbel-key sampler (extension, include/wmar_hip.h wmar_rar_generate_gumbel)."""
        class_ids, out, (sc, sc_ptr, guided) = self._staging(class_ids, cfg_scales)
        _require_cuda(log_rs, "gumbel key")
        assert log_rs.shape == (self.cfg.codebook_size,) and log_rs.dtype == torch.float32 and log_rs.is_contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self._L.wmar_rar_generate_gumbel(
                self._h, class_ids.data_ptr(), class_ids.shape[0], sc_ptr, guided, float(temperature), float(top_p), int(top_k),
                log_rs.data_ptr(), out.data_ptr(), 1 if use_graph else 0, _lib.stream_ptr(self.device)))
            _lib.check(self._L.wmar_rar_check(self._h, _lib.stream_ptr(self.device)))
        return out

    def generate_gumbel_ctx(self, class_ids, h0: int, ngram: int, u: torch.Tensor, cfg_scales, temperature=1.0, top_p=0.0, top_k=0,
                            use_graph=True):
        """RAR.generate with the context-keyed Gumbel sampler (include/wmar_hip.h wmar_rar_generate_gumbel_ctx): ``h0`` the hash of
        the empty window, ``u`` float32 [ngram, B, V] uniform noise of the unkeyed first ``ngram`` positions."""
        class_ids, out, (sc, sc_ptr, guided) = self._staging(class_ids, cfg_scales)
        _require_cuda(u, "u")
        B = class_ids.shape[0]
        assert u.shape == (int(ngram), B, self.cfg.codebook_size) and u.dtype == torch.float32 and u.is_contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self._L.wmar_rar_generate_gumbel_ctx(
                self._h, class_ids.data_ptr(), B, sc_ptr, guided, float(temperature), float(top_p), int(top_k),
                C.c_uint64(int(h0) & 0xFFFFFFFFFFFFFFFF), int(ngram), u.data_ptr(), out.data_ptr(), 1 if use_graph else 0,
                _lib.stream_ptr(self.device)))
            _lib.check(self._L.wmar_rar_check(self._h, _lib.stream_ptr(self.device)))
        return out


class MaskgitVQEngine(_TokenizerEngine):
    """MaskGIT-VQGAN tokenizer of RAR; replaces PretrainedTokenizer.encode / decode_tokens
    (deps/rar/modeling/titok.py:75-89) incl. the wrapper's [-1,1] <-> [0,1] rescaling."""

    _prefix = "wmar_mvq"

    def __init__(self, cfg, state: Dict[str, torch.Tensor], max_batch: int = 64, device="cuda"):
        self.cfg = cfg
        self._out_channels, self._code_dim = cfg.num_channels, cfg.z_channels
        c = _lib.MvqConfig()
        c.hidden_channels, c.num_res_blocks, c.resolution = cfg.hidden_channels, cfg.num_res_blocks, cfg.resolution
        c.num_channels, c.z_channels, c.num_embeddings = cfg.num_channels, cfg.z_channels, cfg.num_embeddings
        c.n_levels = len(cfg.channel_mult)
        for i, m in enumerate(cfg.channel_mult):
            c.channel_mult[i] = m
        c.max_batch = int(max_batch)
        self._create(c, state, lambda k: k.startswith(("encoder.", "decoder.", "quantize.")), device, max_batch)


class ChameleonEngine(_Engine, _GraphCounts):
    """Chameleon / Anole transformer decode with KV cache, three guidance streams and the fused sampler; replaces
    ChameleonModelAdapter + Transformer.forward_with_attn_bias + the ImageDecoder token loop
    (deps/chameleon/inference/model_adapter.py:36-119, transformer.py:288-337, chameleon.py:299-389)."""

    _prefix = "wmar_cham"

    def __init__(self, cfg, state: Dict[str, torch.Tensor], max_batch: int = 16, max_seq_len: int = 1024 + 128, device="cuda"):
        self.cfg = cfg
        self.max_seq_len = int(max_seq_len)
        state = dict(state)
        for l in range(cfg.n_layers):   # the reference's load hooks (transformer.py:84-98, 197-208)
            p = f"layers.{l}."
            if p + "attention.wq.weight" in state:
                state[p + "attention.wqkv.weight"] = torch.cat([state.pop(p + "attention.wq.weight"), state.pop(p + "attention.wk.weight"),
                                                                 state.pop(p + "attention.wv.weight")])
            if p + "feed_forward.w1.weight" in state:
                state[p + "feed_forward.w13.weight"] = torch.cat([state.pop(p + "feed_forward.w1.weight"),
                                                                   state.pop(p + "feed_forward.w3.weight")])
        state.pop("rope.freqs", None)
        dts = {v.dtype for v in state.values()}
        bf16 = dts == {torch.bfloat16}
        c = _lib.ChamConfig(cfg.dim, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, cfg.vocab_size, cfg.ffn_hidden, cfg.norm_eps,
                            cfg.rope_theta, int(cfg.qk_normalization), int(cfg.swin_norm), 3 * int(max_batch), self.max_seq_len,
                            int(bf16))
        self._create(c, state, lambda k: True, device, max_batch, torch.bfloat16 if bf16 else torch.float32)
        torch.cuda.synchronize(self.device)

    def forward_tokens(self, tok: torch.Tensor, pos: torch.Tensor, want_logits: bool = True) -> Optional[torch.Tensor]:
        """tok int64 [M], pos int32 [M] -> logits float32 [M, V] (one token per sequence, warm caches)."""
        _require_cuda(tok, "tokens")
        tok = tok.to(torch.int64).contiguous().view(-1)
        pos = pos.to(device=self.device, dtype=torch.int32).contiguous().view(-1)
        M = tok.shape[0]
        logits = torch.empty(M, self.cfg.vocab_size, dtype=torch.float32, device=self.device) if want_logits else None
        with torch.cuda.device(self.device):
            _lib.check(self._L.wmar_cham_forward_tokens(self._h, tok.data_ptr(), pos.data_ptr(), M,
                                                        logits.data_ptr() if want_logits else None, _lib.stream_ptr(self.device)))
        return logits

    def generate_image(self, prompts, q: torch.Tensor, n_tokens: int, temperature: float, top_p: Optional[float],
                       guidance_scale_text: float, guidance_scale_image: float, allow: Optional[torch.Tensor] = None,
                       wm_ctx: Optional[_lib.WmCtx] = None, use_graph: bool = True,
                       allow_ids: Optional[torch.Tensor] = None, pad_id: int = 1, processor=None) -> torch.Tensor:
        """prompts: the 3B token lists (full-, image-, un-conditioned, in that order); q float32 [n_tokens, B, V];
        allow: int32 bitmap [V/32] of permitted vocabulary entries; allow_ids: the same set as ascending int32 ids (lets the
        sampler work on the compacted row); pad_id: the id short prompts are left-padded with (it can enter the watermark context
        of the first image tokens).  Returns int64 [B, n_tokens] vocabulary ids.  ``generate_image_hooked`` is this call with
        ``processor``: ``processor(input_ids int64 [B, P+n], logits float32 [B, V])``, positional, on the first stream's left-padded
        prompt plus the generated tokens and the logits behind the three-way mix, in front of allow-only."""
        _require_cuda(q, "q")
        M = len(prompts)
        assert M % 3 == 0
        B = M // 3
        V = self.cfg.vocab_size
        assert q.shape == (n_tokens, B, V) and q.dtype == torch.float32 and q.is_contiguous()
        flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int64) for p in prompts]))
        lens = np.ascontiguousarray(np.asarray([len(p) for p in prompts], dtype=np.int32))
        out = torch.empty(B, n_tokens, dtype=torch.int64, device=self.device)
        sp = _lib.ChamSampleParams(float(temperature), float(top_p) if top_p is not None else -1.0, float(guidance_scale_text),
                                   float(guidance_scale_image), 1 if use_graph else 0, int(pad_id))
        if allow is not None:
            _require_cuda(allow, "allow bitmap")
            assert allow.dtype == torch.int32 and allow.numel() == V // 32 and allow.is_contiguous()
        if allow_ids is not None:
            _require_cuda(allow_ids, "allow ids")
            assert allow is not None and allow_ids.dtype == torch.int32 and allow_ids.is_contiguous()
        # what both entry points take between the engine (and the watermark) in front and the hook buffers / the stream behind
        args = (flat.ctypes.data, lens.ctypes.data, B, C.byref(sp), allow.data_ptr() if allow is not None else None,
                allow_ids.data_ptr() if allow_ids is not None else None, int(allow_ids.numel()) if allow_ids is not None else 0,
                q.data_ptr(), int(n_tokens), out.data_ptr())
        with torch.cuda.device(self.device):
            if processor is not None:
                assert wm_ctx is None, "a logit processor replaces the fused watermark"
                hook = _LogitsHook(processor, B, V, int(lens.max()) + int(n_tokens), self.device, positional=True)
                hook.finish(self._L.wmar_cham_generate_image_hooked(
                    self._h, *args, hook.logits.data_ptr(), hook.past.data_ptr(), hook.past.stride(0), hook.cfunc, None,
                    _lib.stream_ptr(self.device)))
            else:
                _lib.check(self._L.wmar_cham_generate_image(self._h, C.byref(wm_ctx) if wm_ctx is not None else None, *args,
                                                            _lib.stream_ptr(self.device)))
        return out

    def generate_image_hooked(self, prompts, q: torch.Tensor, n_tokens: int, processor, temperature: float, top_p: Optional[float],
                              guidance_scale_text: float, guidance_scale_image: float, allow: Optional[torch.Tensor] = None,
                              use_graph: bool = True, allow_ids: Optional[torch.Tensor] = None, pad_id: int = 1) -> torch.Tensor:
        """``generate_image`` with a reference-style logit processor (HF ``LogitsProcessor`` call) between the guidance mix and
        allow-only; see ``generate_image``."""
        return self.generate_image(prompts, q, n_tokens, temperature, top_p, guidance_scale_text, guidance_scale_image, allow=allow,
                                   use_graph=use_graph, allow_ids=allow_ids, pad_id=pad_id, processor=processor)
