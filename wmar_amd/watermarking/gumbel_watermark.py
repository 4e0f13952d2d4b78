"""Gumbel-key ("Aaronson") watermark on MI355X -- SURVEY.md section 8a row G1.

Mirrors ``wmar_audio/watermark/engine.py`` (``get_wm_window_hash`` :13-26, ``gumbel_sample`` :29-75,
``gumbel_score_tok`` :123-134): same names, arguments and return dtypes, tensors on the GPU.  The
reference's image code never calls them; ``GumbelWatermark`` (RAR + Gumbel key, BASELINE config 3)
is therefore an extension: detector = sum of the per-token scores ``-log(1 - rs[token])`` against their Gamma(n, 1) null
distribution.  ``ngram = 0``: one fixed key, every position scored.  ``ngram > 0``: the key of a position is hashed from the
``ngram`` ids in front of it and derived on the device (``wmar_gumbel_key_rows``); the first ``ngram`` positions are unkeyed and a
repeated (ngram+1)-tuple is scored once.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Tuple

import numpy as np
import torch

from .. import _lib


def empty_window_hash(seed: int) -> int:
    """h0 of ``get_wm_window_hash`` for ``ngram > 0``: the first randint of the CPU generator seeded with ``seed``."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return int(torch.randint(0, 2 ** 31 - 1, (1,), generator=g).item())


def get_wm_window_hash(ngrams: torch.Tensor = None, seed: int = 0) -> torch.Tensor:
    """engine.py:13-26.  ``ngram == 0``: the hash is the seed.  ``ngram > 0`` raises TypeError in the reference
    (``GENERATOR=`` keyword, :23); the evident intent -- first randint of the seeded generator xor the tokens --
    is what runs here."""
    batch_size, wm_ngram = ngrams.shape
    if wm_ngram == 0:
        return torch.full((batch_size,), seed, dtype=torch.int64)
    out = torch.full((batch_size,), empty_window_hash(seed), dtype=torch.int64)
    ng = ngrams.detach().to("cpu", torch.int64)
    for ii in range(wm_ngram):
        out ^= ng[:, ii]
    return out


MAX_CONTEXT = 16      # WMAR_MAX_CONTEXT of include/wmar_hip.h

_KEYS: Dict[Tuple[int, int, str], Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}


def key_for(seed: int, vocab_size: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(rs, log rs, -log(1 - rs)) float32 [V] on ``device`` for one window hash."""
    device = torch.device(device)
    k = (int(seed), int(vocab_size), str(device))
    if k not in _KEYS:
        rs = np.zeros(vocab_size, np.float32)
        lr = np.zeros(vocab_size, np.float32)
        sc = np.zeros(vocab_size, np.float32)
        _lib.check(_lib.load().wmar_gumbel_key_build(C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), vocab_size, rs.ctypes.data,
                                                      lr.ctypes.data, sc.ctypes.data))
        _KEYS[k] = tuple(torch.from_numpy(a).to(device) for a in (rs, lr, sc))
        if len(_KEYS) > 4096:
            _KEYS.pop(next(iter(_KEYS)))
    return _KEYS[k]


def key_rows(window_hash: torch.Tensor, vocab_size: int, device, want=(True, True, True)):
    """(rs, log rs, -log(1 - rs)) float32 [N, V] on ``device`` for int64 hashes [N], derived on the device
    (``wmar_gumbel_key_rows``): bit-equal to ``key_for`` of every hash.  ``want``: which of the three to build (others None)."""
    device = torch.device(device)
    wh = window_hash.detach().to(device=device, dtype=torch.int64).contiguous().view(-1)
    out = [torch.empty(wh.numel(), vocab_size, dtype=torch.float32, device=device) if w else None for w in want]
    if wh.numel():
        with torch.cuda.device(device):
            _lib.check(_lib.load().wmar_gumbel_key_rows(wh.data_ptr(), wh.numel(), vocab_size,
                                                        *[t.data_ptr() if t is not None else None for t in out],
                                                        _lib.stream_ptr(device)))
    return tuple(out)


def _key_rows(window_hash: torch.Tensor, vocab_size: int, device, which: int):
    """Key rows for a batch of hashes: ([V] tensor, stride 0) when all rows share one hash, else ([B, V], V) derived on the device
    from the hash tensor as it is.  Hashes that already live on the device are never read back: they take the second form."""
    wh = window_hash.detach().view(-1)
    if not wh.is_cuda and (wh.numel() == 1 or bool((wh == wh[0]).all())):
        return key_for(int(wh[0]), vocab_size, device)[which], 0
    return key_rows(wh, vocab_size, device, tuple(i == which for i in range(3)))[which], vocab_size


def gumbel_sample(logits: torch.Tensor, window_hash: torch.Tensor, use_sampling: bool = False, temp: float = 1.0,
                  top_p: float = 0.0, top_k: int = 0) -> torch.Tensor:
    """engine.py:29-75 for logits float32 [B, V] on the GPU -> next tokens int64 [B]."""
    if not logits.is_cuda:
        raise RuntimeError("gumbel_sample: logits must be on the GPU (wmar_amd has no CPU path)")
    lg = logits.detach().to(torch.float32).contiguous()
    B, V = lg.shape
    out = torch.empty(B, dtype=torch.int64, device=lg.device)
    if B == 0:
        return out
    key, stride = _key_rows(window_hash, V, lg.device, 1)
    with torch.cuda.device(lg.device):
        _lib.check(_lib.load().wmar_gumbel_sample(lg.data_ptr(), B, V, key.data_ptr(), stride, int(bool(use_sampling)), float(temp),
                                                  float(top_p), int(top_k), out.data_ptr(), _lib.stream_ptr(lg.device)))
    return out


def gumbel_score_tok(tokens: torch.Tensor, window_hash: torch.Tensor, vocab_size: int) -> torch.Tensor:
    """engine.py:123-134: tokens int64 [B] -> int64 scores (the reference accumulates into ``zeros_like(tokens)``, so
    ``-log(1 - rs)[token]`` arrives truncated)."""
    if not tokens.is_cuda:
        raise RuntimeError("gumbel_score_tok: tokens must be on the GPU (wmar_amd has no CPU path)")
    tk = tokens.detach().to(torch.int64).contiguous().view(-1)
    out = torch.empty_like(tk)
    if tk.numel() == 0:
        return out
    key, stride = _key_rows(window_hash, vocab_size, tk.device, 2)
    with torch.cuda.device(tk.device):
        _lib.check(_lib.load().wmar_gumbel_score(tk.data_ptr(), tk.numel(), 1, vocab_size, key.data_ptr(), stride, out.data_ptr(),
                                                 None, _lib.stream_ptr(tk.device)))
    return out


class GumbelWatermark:
    """Gumbel-key watermark for an image-token model (extension, see module docstring).  ``ngram = 0``: one fixed key."""

    def __init__(self, vocab_size: int, seed: int = 42, temperature: float = 1.0, top_p: float = 0.0, top_k: int = 0,
                 device="cuda", ngram: int = 0):
        self.vocab_size = int(vocab_size)
        self.seed = int(seed)
        self.temperature, self.top_p, self.top_k = float(temperature), float(top_p), int(top_k)
        self.device = torch.device(device)
        self.ngram = int(ngram)
        if self.ngram < 0 or self.ngram > MAX_CONTEXT:
            raise ValueError(f"GumbelWatermark: ngram {ngram} outside 0..{MAX_CONTEXT}")
        if self.ngram > 0:
            if self.vocab_size > 16384:
                raise ValueError("GumbelWatermark: ngram > 0 needs a vocabulary of at most 16384 entries")
            self.h0 = empty_window_hash(self.seed)
        else:
            self.rs, self.log_rs, self.score_key = key_for(self.seed, self.vocab_size, self.device)

    def __str__(self):
        s = f"gumbel_seed={self.seed}_T={self.temperature}_topp={self.top_p}_topk={self.top_k}"
        return s + f"_ngram={self.ngram}" if self.ngram > 0 else s

    def sample(self, logits: torch.Tensor, context: torch.Tensor = None) -> torch.Tensor:
        """Next tokens for logits [B, V]; with ``ngram > 0`` ``context`` int64 [B, ngram] holds the ids in front."""
        if self.ngram > 0:
            if context is None or tuple(context.shape) != (logits.shape[0], self.ngram):
                raise ValueError(f"GumbelWatermark.sample: context [B, {self.ngram}] required")
            h = get_wm_window_hash(context, self.seed)
        else:
            h = torch.full((logits.shape[0],), self.seed, dtype=torch.int64)
        return gumbel_sample(logits, h, True, self.temperature, self.top_p, self.top_k)

    def score_counts(self, codes: torch.Tensor):
        """(scores float32 [B, L] (0 where unscored), scored mask int8 [B, L], n_scored int32 [B]) on the device."""
        codes = codes.to(self.device, torch.int64).contiguous()
        B, L = codes.shape
        out = torch.empty(B, L, dtype=torch.float32, device=self.device)
        if self.ngram == 0:
            if B:
                with torch.cuda.device(self.device):
                    _lib.check(_lib.load().wmar_gumbel_score(codes.data_ptr(), B, L, self.vocab_size, self.score_key.data_ptr(), 0,
                                                             None, out.data_ptr(), _lib.stream_ptr(self.device)))
            return (out, torch.ones(B, L, dtype=torch.int8, device=self.device),
                    torch.full((B,), L, dtype=torch.int32, device=self.device))
        mask = torch.empty(B, L, dtype=torch.int8, device=self.device)
        ns = torch.empty(B, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().wmar_gumbel_score_ctx(codes.data_ptr(), B, L, self.vocab_size, C.c_uint64(self.h0), self.ngram,
                                                         out.data_ptr(), mask.data_ptr(), ns.data_ptr(),
                                                         _lib.stream_ptr(self.device)))      # L <= ngram: ValueError
        return out, mask, ns

    def scores(self, codes: torch.Tensor) -> torch.Tensor:
        """float32 [B, L] per-token scores -log(1 - rs[code]) (``ngram > 0``: of the position's own key, 0 where unscored)."""
        return self.score_counts(codes)[0]

    def detect_counts(self, codes: torch.Tensor):
        """(p-values float64 [B], n_scored int32 [B]): under H0 the scored entries are i.i.d. Exp(1), so their sum is
        Gamma(n_scored, 1)."""
        s, _, ns = self.score_counts(codes)
        return torch.special.gammaincc(ns.to(torch.float64), s.to(torch.float64).sum(dim=1)), ns

    def detect(self, codes: torch.Tensor) -> torch.Tensor:
        return self.detect_counts(codes)[0]
