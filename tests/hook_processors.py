"""Reference-style logit processors and the oracle loops that run them -- shared by tests/golden/make_hook_vectors.py,
tests/test_hook_reference.py (CPU) and tests/test_gpu_hook.py.

The processors are device-agnostic torch code: integer arithmetic on the ids, and fp32 additions of constants that are exact in fp32
(an IEEE addition rounds the same way everywhere), so the CPU oracle and the GPU agree bit for bit.  All of them take
``(past_ids, logits)`` -- callable by keyword as Taming / RAR call their processor (mingpt.py:348-350, rar.py:450-451) and
positionally as HF's ``LogitsProcessorList`` calls Chameleon's.

The oracle loops compose the committed oracles (oracle/*.py) with a processor at the point where the reference calls it.  ``jitter``
(nullable: ``(step, logits) -> logits``) perturbs the model's logits in front of the processor; the fixture script uses it to show
that no recorded decision sits on a knife edge.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import cham_oracle as CO
from oracle import model_oracle as M
from oracle import rar_oracle as R
from oracle import wm_oracle as W


# ------------------------------------------------------------------------------------------------------------ processors
def greenlist_from_table(wm):
    """(a) GentimeWatermark's bias (gentime_watermark.py:229-271) written in torch from the key table of ``wm``
    (``key_table_host()``; FIXED / LINEAR seeding): ``delta`` is added where the bit of table row ``sum(past_ids[:, -h:])`` is set;
    rows whose context is too short are left alone."""
    table = torch.from_numpy(wm.key_table_host().view(np.int32))
    h, delta, V = int(wm.context_size), float(wm.delta), int(wm.vocab_size)
    fixed = table.shape[0] == 1
    cache = {}

    def processor(past_ids, logits):
        if not fixed and past_ids.shape[1] < h:
            return logits
        tab = cache.get(logits.device)
        if tab is None:
            tab = cache[logits.device] = table.to(logits.device)
        row = torch.zeros(logits.shape[0], dtype=torch.int64, device=logits.device) if fixed else \
            past_ids[:, past_ids.shape[1] - h:].sum(dim=1).to(logits.device)
        words = tab[row]                                                                  # [B, V / 32]
        shifts = torch.arange(32, dtype=torch.int32, device=logits.device)
        green = ((words[:, :, None] >> shifts) & 1).reshape(logits.shape[0], -1)[:, :V].bool()
        logits.copy_(torch.where(green, logits + delta, logits))
        return logits

    return processor


def hash_bias(past_ids, logits):
    """(b) +3.0 where (id * 2654435761 + sum of the last two context ids) mod 5 == 0, -1.5 where it is 1."""
    V = logits.shape[1]
    ctx = past_ids[:, max(past_ids.shape[1] - 2, 0):].sum(dim=1).to(logits.device)       # [B]; 0 for an empty context
    ids = torch.arange(V, dtype=torch.int64, device=logits.device)
    r = (ids[None, :] * 2654435761 + ctx[:, None]) % 5
    logits.copy_(torch.where(r == 0, logits + 3.0, torch.where(r == 1, logits - 1.5, logits)))
    return logits


def ban_repeats(past_ids, logits):
    """(c) every id already in ``past_ids`` -- the whole growing context -- is set to -inf."""
    if past_ids.shape[1] > 0:
        logits.scatter_(1, past_ids.to(logits.device), float("-inf"))
    return logits


def out_of_place(p):
    """(d) ``p`` on a copy: returns a NEW tensor and leaves the buffer it was handed untouched."""
    def processor(past_ids, logits):
        return p(past_ids, logits.clone())
    return processor


def identity(past_ids, logits):
    return logits


PROCESSORS = {"hash": lambda: hash_bias, "ban": lambda: ban_repeats, "oop_hash": lambda: out_of_place(hash_bias)}


def uniform_jitter(seed: int, amp: float = 5e-4):
    """Seeded uniform noise of +-amp on every step's logits (5e-4: the logit tolerance tests/test_gpu_gpt.py grants the engine)."""
    g = torch.Generator().manual_seed(seed)

    def jitter(step, logits):
        return logits + (torch.rand(logits.shape, generator=g, dtype=torch.float32) * 2 - 1) * amp
    return jitter


# ------------------------------------------------------------------------------------------------------------ oracle loops
@torch.no_grad()
def taming_loop(sd, n_head, cond, steps, processor, temperature=1.0, top_k=None, top_p=None, q=None, jitter=None):
    """sample_with_past (mingpt.py:326-368): oracle.model_oracle.gpt_step -> processor(past_ids=, logits=) -> wm_oracle.sample_rows.
    cond int64 [B, 1]; q float32 [steps, B, V] (None: drawn from the default CPU generator step by step, as torch.multinomial).
    Returns int64 [B, steps] (numpy)."""
    sample = cond.clone()
    pk = pv = None
    x = cond
    V = sd["head.weight"].shape[0]
    for n in range(steps):
        logits, nk, nv = M.gpt_step(sd, n_head, x, pk, pv, n)
        pk = nk if pk is None else [torch.cat((a, b), dim=-2) for a, b in zip(pk, nk)]
        pv = nv if pv is None else [torch.cat((a, b), dim=-2) for a, b in zip(pv, nv)]
        logits = logits.clone()
        if jitter is not None:
            logits = jitter(n, logits)
        if processor is not None:
            logits = processor(past_ids=sample, logits=logits).to(torch.float32)
        qn = q[n] if q is not None else torch.empty(cond.shape[0], V, dtype=torch.float32).exponential_(1)
        tok = W.sample_rows(logits.numpy(), np.asarray(qn, dtype=np.float32), temperature, top_k, top_p)
        x = torch.from_numpy(tok).view(-1, 1)
        sample = torch.cat((sample, x), dim=1)
    return sample[:, 1:].numpy()


@torch.no_grad()
def rar_loop(sd, cfg, condition, processor, guidance_scale=4.0, guidance_scale_pow=0.0, temperature=1.0, jitter=None):
    """RAR.generate (rar.py:408-459) as oracle.rar_oracle.generate with a ``sampler`` that runs the processor on the mixed logits
    and the generated ids so far.  The noise comes from the default CPU generator in the reference's order (label-drop mask, then one
    [B, V] exponential per step).  Returns int64 [B, L] (numpy)."""
    B, V = condition.shape[0], cfg.codebook_size
    ids = [torch.zeros(B, 0, dtype=torch.long)]

    def sampler(mixed, step):
        lg = mixed.clone()
        if jitter is not None:
            lg = jitter(step, lg)
        if processor is not None:
            lg = processor(past_ids=ids[0], logits=lg).to(torch.float32)
        qn = torch.empty(B, V, dtype=torch.float32).exponential_(1)
        tok = torch.from_numpy(W.sample_rows(lg.numpy(), qn.numpy(), temperature, None, None))
        ids[0] = torch.cat([ids[0], tok.view(-1, 1)], dim=1)
        return tok

    return R.generate(sd, cfg, condition, guidance_scale, guidance_scale_pow, temperature, sampler=sampler).numpy()


@torch.no_grad()
def cham_loop(sd, cfg, prompts3, n_tokens, processor, q, temperature, top_p, g_text, g_image, allow_ids, pad_id, forward=None):
    """ImageDecoder (chameleon.py:299-389) for the 3B prompt lists ``prompts3``: cham_oracle.forward_tokens + instruct_cfg ->
    processor(input_ids, logits), positional, on the first stream's left-padded rows -> allow-only -> temperature -> top-p ->
    sample_rows.  q float32 [n_tokens, B, V].  ``forward``: None = the oracle's own transformer (fold=True: the engine's algebra);
    or a callable ``(tok int64 [3B], pos int32 [3B]) -> logits [3B, V]`` fed the right-aligned prompt first.  Returns int64 [B, n_tokens]."""
    M3 = len(prompts3)
    B = M3 // 3
    maxlen = max(len(p) for p in prompts3)
    if forward is None:
        cache = CO.Cache(cfg.n_layers, M3)
        lg, _ = CO.prefill_right_aligned(sd, cfg, prompts3, cache, fold=True)

        def forward(tok, pos):
            return CO.forward_tokens(sd, cfg, tok, pos, cache, fold=True)
    else:
        lg = None
        for j in range(maxlen):
            tok = [p[j - (maxlen - len(p))] if j - (maxlen - len(p)) >= 0 else 0 for p in prompts3]
            pos = [max(j - (maxlen - len(p)), 0) for p in prompts3]
            lg = forward(torch.tensor(tok, dtype=torch.int64), torch.tensor(pos, dtype=torch.int32))
    past = torch.tensor([[pad_id] * (maxlen - len(p)) + list(p) for p in prompts3[:B]], dtype=torch.int64)
    pos = torch.tensor([len(p) for p in prompts3], dtype=torch.int32)
    keep = np.zeros(cfg.vocab_size, dtype=bool)
    keep[np.asarray(allow_ids)] = True
    out = []
    for n in range(n_tokens):
        mixed = CO.instruct_cfg(lg.float().cpu(), g_text, g_image).clone()
        if processor is not None:
            mixed = processor(past, mixed).to(torch.float32)
        x = mixed.numpy().copy()
        x[:, ~keep] = -np.inf
        tok = W.sample_rows(x, np.asarray(q[n], dtype=np.float32), temperature, None, top_p)
        out.append(tok)
        t = torch.from_numpy(tok)
        past = torch.cat([past, t.view(-1, 1)], dim=1)
        if n < n_tokens - 1:
            lg = forward(torch.cat([t, t, t]), pos + n)
    return np.stack(out, axis=1)


# ------------------------------------------------------------------------------------------------------------ fixture cases
TAMING_SETTINGS = {"k250p92": (250, 0.92, 1.0), "plain": (None, None, 1.0)}     # of tests/test_gpu_gpt.py's LOOPS
TAMING_COND = [[7], [980], [1], [340]]                                            # golden["loop_cond"]
RAR_CLASSES = [3, 977, 0, 512]                                                    # rar_vectors["rar_cond"]
