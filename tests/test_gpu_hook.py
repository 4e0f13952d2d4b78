"""The hooked generation mode of the three engines: a reference-style logit processor between the model step and the sampler.

1. the reference's tokens through the hook; 2. hooked == fused bit for bit on every launch plan; 3. wmar_cfg_mix; 4. the processor
contract; 5. how the wrappers choose the loop; 6. re-run behind a failed barrier and graph reuse."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import rar_oracle as R  # noqa: E402
from tests import hook_processors as HP  # noqa: E402
from tests.conftest import REPO  # noqa: E402
from tests.test_gpu_watermark import _wm  # noqa: E402
from wmar_amd.utils import synth  # noqa: E402

SMALL = synth.GPTConfig(vocab_size=16384, block_size=16, n_layer=2, n_head=4, n_embd=128)
LOOPS = {"k250p92": (250, 0.92, 1.0), "k100p80T13": (100, 0.8, 1.3), "nok_p95": (None, 0.95, 0.9),
         "k50nop": (50, None, 1.0), "plain": (None, None, 1.0)}
PROD = synth.GPTConfig(vocab_size=16384, block_size=16, n_layer=2, n_head=24, n_embd=1536)        # production width, two layers
RCFG = synth.RARConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                       image_seq_len=16, codebook_size=1024, condition_num_classes=1000)
RXL = synth.RARConfig(hidden_size=1280, num_hidden_layers=2, num_attention_heads=16, intermediate_size=5120,
                      image_seq_len=16, codebook_size=1024, condition_num_classes=1000)            # RAR-XL width, two layers


@pytest.fixture(scope="module")
def hv():
    return np.load(os.path.join(REPO, "tests", "golden", "hook_vectors.npz"))


@pytest.fixture(scope="module")
def rv():
    return np.load(os.path.join(REPO, "tests", "golden", "rar_vectors.npz"))


@pytest.fixture(scope="module")
def small_engine():
    from wmar_amd.models.engine import GPTEngine
    return GPTEngine(SMALL, synth.synth_gpt_state(SMALL, seed=3, logit_scale=40.0), max_batch=64)


@pytest.fixture(scope="module")
def prod_engine():
    from wmar_amd.models.engine import GPTEngine
    return GPTEngine(PROD, synth.synth_gpt_state_fast(PROD, seed=1, device="cuda", logit_scale=10.0), max_batch=128)


@pytest.fixture(scope="module")
def rar_small():
    from wmar_amd.models.engine import RAREngine
    return RAREngine(RCFG, synth.synth_rar_state(RCFG, seed=2, logit_scale=30.0), max_batch=8)


@pytest.fixture(scope="module")
def rar_xl():
    from wmar_amd.models.engine import RAREngine
    return RAREngine(RXL, synth.synth_rar_state(RXL, seed=5, device="cuda", logit_scale=20.0, gen_device="cuda"), max_batch=64)


@pytest.fixture(scope="module")
def wm_taming(kat):
    wm = _wm(kat["keys"]["taming"])
    return wm, HP.greenlist_from_table(wm)


@pytest.fixture(scope="module")
def wm_rar(kat):
    wm = _wm(kat["keys"]["rar"])
    return wm, HP.greenlist_from_table(wm)


def _cpu_noise(seed, steps, B, V, drop_mask=False):
    """the noise torch.multinomial drew in the reference's CPU run"""
    torch.manual_seed(seed)
    if drop_mask:
        torch.rand(B, 1)
    return torch.stack([torch.empty(B, V).exponential_(1) for _ in range(steps)]).cuda()


def _gpu_noise(seed, steps, B, V):
    return torch.empty(steps, B, V, device="cuda").exponential_(1, generator=torch.Generator(device="cuda").manual_seed(seed))


# ------------------------------------------------------------------------------------- 1. reference tokens through the hook
@pytest.mark.parametrize("tag", list(LOOPS))
@pytest.mark.parametrize("graph", [True, False])
def test_taming_greenlist_processor_reproduces_reference_tokens(golden, small_engine, wm_taming, tag, graph):
    tk, tp, T = LOOPS[tag]
    q = _cpu_noise(11, 16, 4, 16384)
    toks = small_engine.generate_hooked(torch.from_numpy(golden["loop_cond"]).view(-1).cuda(), 16, q, wm_taming[1], T, tk, tp,
                                        use_graph=graph)
    assert np.array_equal(toks.cpu().numpy(), golden[f"loop_{tag}_tokens"])


@pytest.mark.parametrize("graph", [True, False])
def test_rar_greenlist_processor_reproduces_reference_tokens(rv, rar_small, wm_rar, graph):
    q = _cpu_noise(21, 16, 4, 1024, drop_mask=True)
    toks = rar_small.generate_hooked(torch.from_numpy(rv["rar_cond"]).cuda(), q, R.cfg_scales(16, 4.0, 0.0), wm_rar[1], 1.0,
                                     use_graph=graph)
    assert np.array_equal(toks.cpu().numpy(), rv["rar_tokens_wm"])


@pytest.mark.parametrize("proc", list(HP.PROCESSORS))
@pytest.mark.parametrize("tag", list(HP.TAMING_SETTINGS))
@pytest.mark.parametrize("graph", [True, False])
def test_taming_foreign_processors_reproduce_reference_tokens(hv, small_engine, tag, proc, graph):
    tk, tp, T = HP.TAMING_SETTINGS[tag]
    q = _cpu_noise(int(hv["taming_noise_seed"]), 16, 4, 16384)
    toks = small_engine.generate_hooked(torch.tensor(HP.TAMING_COND).view(-1).cuda(), 16, q, HP.PROCESSORS[proc](), T, tk, tp,
                                        use_graph=graph)
    assert np.array_equal(toks.cpu().numpy(), hv[f"taming_{tag}_{proc}"])


@pytest.mark.parametrize("proc", list(HP.PROCESSORS))
@pytest.mark.parametrize("graph", [True, False])
def test_rar_foreign_processors_reproduce_reference_tokens(hv, rar_small, proc, graph):
    q = _cpu_noise(int(hv["rar_noise_seed"]), 16, 4, 1024, drop_mask=True)
    toks = rar_small.generate_hooked(torch.tensor(HP.RAR_CLASSES).cuda(), q, R.cfg_scales(16, 4.0, 0.0), HP.PROCESSORS[proc](), 1.0,
                                     use_graph=graph)
    assert np.array_equal(toks.cpu().numpy(), hv[f"rar_{proc}"])


# ------------------------------------------------------------------------------------- 2. hooked == fused, every plan
@pytest.mark.parametrize("B", [1, 5, 16, 33, 64, 128])     # small-batch plan (1, 5) / 13..32 / fused projection / above 64
def test_taming_hooked_equals_fused_on_every_plan(prod_engine, wm_taming, B):
    """production width (24 heads x 64, n_embd 1536, V 16384), two layers: processor (a) == the fused key table, identity == no
    watermark, bit for bit, graph and eager"""
    wm, green = wm_taming
    cond = (torch.arange(B) * 37 % 1000).cuda()
    q = _gpu_noise(B, 16, B, 16384)
    fused = prod_engine.generate(cond, 16, q, 1.0, 250, 0.92, wm.wm_ctx())
    plain = prod_engine.generate(cond, 16, q, 1.0, 250, 0.92, None)
    assert not torch.equal(fused, plain)
    for graph in (True, False):
        assert torch.equal(prod_engine.generate_hooked(cond, 16, q, green, 1.0, 250, 0.92, use_graph=graph), fused), graph
        assert torch.equal(prod_engine.generate_hooked(cond, 16, q, HP.identity, 1.0, 250, 0.92, use_graph=graph), plain), graph
    assert prod_engine.plan_info(B)["barrier_fallbacks"] == "0"


@pytest.mark.parametrize("which,B", [("small", 4), ("xl", 64)])     # 128 rows under guidance at RAR-XL width
def test_rar_hooked_equals_fused(rar_small, rar_xl, wm_rar, which, B):
    wm, green = wm_rar
    e = rar_small if which == "small" else rar_xl
    cls = (torch.arange(B) * 13 % 1000).cuda()
    q = _gpu_noise(100 + B, 16, B, 1024)
    sc = R.cfg_scales(16, 4.0, 0.0)
    fused, plain = e.generate(cls, q, sc, 1.0, wm.wm_ctx()), e.generate(cls, q, sc, 1.0, None)
    assert not torch.equal(fused, plain)
    for graph in (True, False):
        assert torch.equal(e.generate_hooked(cls, q, sc, green, 1.0, use_graph=graph), fused), graph
        assert torch.equal(e.generate_hooked(cls, q, sc, HP.identity, 1.0, use_graph=graph), plain), graph
    # without guidance the position writes the caller's buffer directly
    assert torch.equal(e.generate_hooked(cls, q, None, green, 0.9), e.generate(cls, q, None, 0.9, wm.wm_ctx()))
    assert e.launch_status()["fallbacks"] == 0


def _cham_small(max_batch=3):
    from wmar_amd.models.chameleon_wrapper import ChameleonARMMWrapper
    cfg = synth.ChameleonConfig(dim=256, n_layers=2, n_heads=4, n_kv_heads=4, vocab_size=2048, multiple_of=64)
    vq_cfg = synth.VQConfig(ch=32, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(), resolution=16, z_channels=32, embed_dim=32,
                            n_embed=512)
    sd = synth.synth_chameleon_state(cfg, seed=8, logit_scale=6.0)
    m = ChameleonARMMWrapper(None, 0, cfg=cfg, state=sd, vocab_map=synth.synth_chameleon_vocab(2048, 512), vq_cfg=vq_cfg,
                             vq_state=synth.synth_vq_state(vq_cfg, 1), max_batch=max_batch, max_prompt_len=16)
    return m, cfg, sd


@pytest.fixture(scope="module")
def cham():
    m, cfg, sd = _cham_small()
    text = m.vocab.text_tokens
    cond = [(0, [text[5], text[9], text[100]]), (1, [text[7]]), (2, [text[1], text[2], text[3], text[4], text[400]])]   # unequal lengths
    return m, cfg, sd, cond


@pytest.mark.parametrize("h", [1, 2])
def test_chameleon_hooked_equals_fused(cham, h):
    """2 layers, dim 256, prompts of unequal length: processor (a) on the whole left-padded row == the fused key table (h = 2: the
    first token's context reaches into the prompt), identity == no watermark; graph and eager"""
    from wmar_amd.watermarking.gentime_watermark import GentimeWatermark, SeedStrategy, SplitStrategy
    m, cfg, sd, cond = cham
    wm = GentimeWatermark(m.get_vq(), 2048, SeedStrategy.LINEAR, SplitStrategy.RANDOM_STRATIFIED, h, 3.0, 0.25, device="cuda")
    green = HP.greenlist_from_table(wm)
    gp = {"temperature": 0.9, "top_p": 0.8}
    torch.manual_seed(3)
    q = m.draw_noise(3)
    m.set_watermarker(wm)
    m.use_graph = True
    fused = m.sample(cond, gp, apply_watermark=True, q=q)
    plain = m.sample(cond, gp, apply_watermark=False, q=q)
    assert not torch.equal(fused, plain)
    for graph in (True, False):
        m.use_graph = graph
        assert torch.equal(m.sample(cond, gp, q=q, logit_processor=green), fused), graph
        assert torch.equal(m.sample(cond, gp, q=q, logit_processor=HP.identity), plain), graph
    m.use_graph = True
    m.set_watermarker(None)


def test_chameleon_hooked_equals_fused_at_7b_width():
    from wmar_amd.models.engine import ChameleonEngine
    from wmar_amd.models.chameleon_wrapper import allow_bitmap
    from wmar_amd.watermarking.gentime_watermark import GentimeWatermark, SeedStrategy, SplitStrategy
    cfg = synth.ChameleonConfig(n_layers=2)
    sd = synth.synth_chameleon_state(cfg, seed=7, device="cuda", logit_scale=4.0, gen_device="cuda")
    e = ChameleonEngine(cfg, sd, max_batch=2, max_seq_len=32)
    V = cfg.vocab_size
    img = list(range(4, 4 + 8192))
    vq = {"alive_ids": torch.tensor(img), "dead_ids": torch.tensor(sorted(set(range(V)) - set(img))), "embedding": None}
    wm = GentimeWatermark(vq, V, SeedStrategy.FIXED, SplitStrategy.RANDOM_STRATIFIED, 0, 3.0, 0.25, device="cuda")   # one table row
    green = HP.greenlist_from_table(wm)
    allow, ids = allow_bitmap(img, V, "cuda"), torch.tensor(img, dtype=torch.int32).cuda()
    full = [[9000, 9001, 9002, 9003], [9100, 9101]]
    prompts = full + [p[-1:] for p in full] + [[9500], [9500]]
    n = 6
    q = _gpu_noise(77, n, 2, V)
    kw = dict(allow=allow, allow_ids=ids, pad_id=1)
    fused = e.generate_image(prompts, q, n, 0.9, 0.8, 3.0, 1.2, wm_ctx=wm.wm_ctx(), **kw)
    plain = e.generate_image(prompts, q, n, 0.9, 0.8, 3.0, 1.2, **kw)
    assert not torch.equal(fused, plain)
    for graph in (True, False):
        assert torch.equal(e.generate_image_hooked(prompts, q, n, green, 0.9, 0.8, 3.0, 1.2, use_graph=graph, **kw), fused), graph
        assert torch.equal(e.generate_image_hooked(prompts, q, n, HP.identity, 0.9, 0.8, 3.0, 1.2, use_graph=graph, **kw), plain), graph
    # no row compaction: the allow-only bitmap alone, behind the hook
    assert torch.equal(e.generate_image_hooked(prompts, q, n, green, 0.9, 0.8, 3.0, 1.2, allow=allow, pad_id=1),
                       e.generate_image(prompts, q, n, 0.9, 0.8, 3.0, 1.2, wm_ctx=wm.wm_ctx(), allow=allow, pad_id=1))


def test_chameleon_hash_processor_equals_the_composed_oracle_loop(cham):
    """Chameleon has no reference fixture (its transformer is not importable offline): processor (b) through the hook == the composed
    loop of tests/hook_processors.cham_loop -- instruct_cfg -> processor -> allow-only -> sample_rows.  The model logits of that loop
    come from a second engine fed the same prompts and tokens, as tests/test_gpu_chameleon.py replays its loop: the bf16 engine agrees
    with cham_oracle.forward_tokens to a tolerance only (3 % of the logit spread, amplified five times by the guidance mix), and with
    perturbations of that size no noise seed keeps all tokens of the oracle's own loop in place, so exact tokens cannot be demanded
    from the oracle's transformer.  Everything behind the model step is the oracle's."""
    from wmar_amd.models.engine import ChameleonEngine
    m, cfg, sd, cond = cham
    gp = {"temperature": 0.9, "top_p": 0.8}
    torch.manual_seed(4)
    q = m.draw_noise(3)
    codes = m.sample(cond, gp, q=q, logit_processor=HP.hash_bias)
    prompts = m.split_inputs_for_cfg([m.tokens_from_ui([{"type": "ids", "value": p}, {"type": "sentinel", "value": "<END-OF-TURN>"}])
                                      for _, p in cond])
    e2 = ChameleonEngine(cfg, sd, max_batch=3, max_seq_len=16 + 64)
    ref = HP.cham_loop(sd, cfg, prompts, 64, HP.hash_bias, q.cpu().numpy(), 0.9, 0.8, m.guidance_scale_text, m.guidance_scale_image,
                       m.vocab.image_tokens, m.vocab.pad_id, forward=lambda tok, pos: e2.forward_tokens(tok.cuda(), pos.cuda()).cpu())
    assert np.array_equal(codes.cpu().numpy(), ref)
    assert not torch.equal(codes, m.sample(cond, gp, q=q))


# ------------------------------------------------------------------------------------------------------ 3. wmar_cfg_mix
def _mix(cond, img, unc, scale=None, step=None, g_text=0.0, g_image=0.0):
    from wmar_amd import _lib
    out = torch.empty_like(cond)
    _lib.check(_lib.load().wmar_cfg_mix(cond.data_ptr(), img.data_ptr() if img is not None else None, unc.data_ptr(), out.data_ptr(),
                                        cond.shape[0], cond.shape[1], scale.data_ptr() if scale is not None else None,
                                        step.data_ptr() if step is not None else None, g_text, g_image, _lib.stream_ptr()))
    return out


@pytest.mark.parametrize("V", [1024, 16384, 65536, 1023, 4098])      # 1023, 4098: rows that are not 16-byte aligned -> scalar form
def test_cfg_mix_equals_the_torch_expression(V):
    g = torch.Generator(device="cuda").manual_seed(V)
    B = 5
    c, i, u = (torch.randn(B, V, device="cuda", generator=g) * 7 for _ in range(3))
    scales = torch.tensor([1.0, 1.5, 2.25, 3.1, 4.0, 0.3, 7.7, 1.0], device="cuda")
    for s in (0, 3, 6):
        step = torch.tensor([s], dtype=torch.int32, device="cuda")            # the scale is read through the device step counter
        want = u + (c - u) * scales[s]
        assert torch.equal(_mix(c, None, u, scales, step).view(torch.int32), want.view(torch.int32)), s
    assert torch.equal(_mix(c, None, u, scales[4:]).view(torch.int32), (u + (c - u) * scales[4]).view(torch.int32))   # no counter: [0]
    want3 = u + 1.2 * (i - u) + 3.0 * (c - i)
    assert torch.equal(_mix(c, i, u, g_text=3.0, g_image=1.2).view(torch.int32), want3.view(torch.int32))
    # a misaligned (but V % 4 == 0) view takes the scalar form too
    if V % 4 == 0:
        big = torch.randn(3, B * V + 1, device="cuda", generator=g)
        c2, u2 = big[0, 1:].view(B, V), big[1, 1:].view(B, V)
        assert torch.equal(_mix(c2, None, u2, scales).view(torch.int32), (u2 + (c2 - u2) * scales[0]).view(torch.int32))


# --------------------------------------------------------------------------------------------------------- 4. contract
class Recorder:
    """records how it was called and what it saw, at every step; edits nothing unless `inner` does"""

    def __init__(self, inner=None):
        self.calls, self.inner = [], inner

    def __call__(self, *args, **kwargs):
        past, logits = (args if args else (kwargs["past_ids"], kwargs["logits"]))
        self.calls.append(dict(n_args=len(args), kw=sorted(kwargs), past=past.clone(), past_shape=tuple(past.shape),
                               past_stride=past.stride(), past_dtype=past.dtype, past_dev=past.device.type,
                               logits_shape=tuple(logits.shape), logits_contig=logits.is_contiguous(), logits_dtype=logits.dtype,
                               logits_ptr=logits.data_ptr(), grad=torch.is_grad_enabled(), logits=logits.clone()))
        return self.inner(past, logits) if self.inner is not None else logits


def _check_calls(rec, B, V, widths, keyword):
    assert len(rec.calls) == len(widths)
    for c, w in zip(rec.calls, widths):
        assert (c["n_args"], c["kw"]) == ((0, ["logits", "past_ids"]) if keyword else (2, []))
        assert c["past_shape"] == (B, w) and c["past_dtype"] == torch.int64 and c["past_dev"] == "cuda"
        assert c["past_stride"] == (widths[-1] + 1, 1)          # a view of the [B, longest + 1] buffer the engine appends to
        assert c["logits_shape"] == (B, V) and c["logits_contig"] and c["logits_dtype"] == torch.float32
        assert c["logits_ptr"] == rec.calls[0]["logits_ptr"] and c["grad"] is False


def test_taming_processor_contract(small_engine):
    """f(past_ids=[B, n+1] class token + generated tokens, logits=raw head output [B, V]), by keyword"""
    B, steps = 5, 16
    cond = torch.tensor([7, 980, 1, 340, 55]).cuda()
    q = _gpu_noise(9, steps, B, 16384)
    rec = Recorder()
    toks, trace = small_engine.generate(cond, steps, q, 1.0, 250, 0.92, None, trace_logits=True)
    got = small_engine.generate_hooked(cond, steps, q, rec, 1.0, 250, 0.92)
    assert torch.equal(got, toks)
    _check_calls(rec, B, 16384, [n + 1 for n in range(steps)], keyword=True)
    for n, c in enumerate(rec.calls):
        assert torch.equal(c["past"], torch.cat([cond[:, None], got[:, :n]], dim=1)), n
        assert torch.equal(c["logits"], trace[n]), n          # the raw head output, bit for bit


def test_rar_processor_contract(rar_small):
    """f(past_ids=[B, n] generated tokens only ([B, 0] first), logits=after guidance, before temperature), by keyword"""
    B = 3
    cls = torch.tensor([3, 977, 0]).cuda()
    q = _gpu_noise(10, 16, B, 1024)
    sc = R.cfg_scales(16, 4.0, 0.0)
    rec = Recorder()
    got = rar_small.generate_hooked(cls, q, sc, rec, 0.7)
    assert torch.equal(got, rar_small.generate(cls, q, sc, 0.7, None))
    _check_calls(rec, B, 1024, list(range(16)), keyword=True)
    # the logits are the guidance mix of the step's conditional / unconditional rows, in front of the temperature: the positions
    # replayed with the tokens returned give them (to the engine's logit tolerance times the guidance scale: the replay takes the
    # unconditional rows' modulation from a GEMM, the loop from its table), and the oracle sampler at T = 0.7 on them gives the tokens
    from oracle import wm_oracle as W
    cond_ids = torch.cat([cls + 1024 + 1, torch.full_like(cls, RCFG.none_condition_id)])
    rar_small.forward_position(torch.full((2 * B,), -1, dtype=torch.int64).cuda(), cond_ids, 0)
    tok = cond_ids
    for n, c in enumerate(rec.calls):
        assert torch.equal(c["past"], got[:, :n]), n
        lg = rar_small.forward_position(tok, cond_ids, n + 1)
        want = lg[B:] + (lg[:B] - lg[B:]) * sc[n].cuda()
        assert float((c["logits"] - want).abs().max()) <= 5e-4 * (1 + 2 * float(sc[n])), n
        assert W.sample_rows(c["logits"].cpu().numpy(), q[n].cpu().numpy(), 0.7, None, None).tolist() == got[:, n].tolist(), n
        tok = torch.cat([got[:, n], got[:, n]])


def test_chameleon_processor_contract(cham):
    """f(input_ids, logits), positional: input_ids = [B, P+n] the first stream's prompt left-padded with pad_id + generated tokens"""
    m, cfg, sd, cond = cham
    gp = {"temperature": 0.9, "top_p": 0.8}
    torch.manual_seed(5)
    q = m.draw_noise(3)
    rec = Recorder()
    got = m.sample(cond, gp, q=q, logit_processor=rec)
    assert torch.equal(got, m.sample(cond, gp, q=q))
    prompts = m.split_inputs_for_cfg([m.tokens_from_ui([{"type": "ids", "value": p}, {"type": "sentinel", "value": "<END-OF-TURN>"}])
                                      for _, p in cond])
    P = max(len(p) for p in prompts)
    _check_calls(rec, 3, 2048, [P + n for n in range(64)], keyword=False)
    padded = torch.tensor([[m.vocab.pad_id] * (P - len(p)) + list(p) for p in prompts[:3]]).cuda()
    assert any(len(p) < P for p in prompts[:3])
    for n, c in enumerate(rec.calls):
        assert torch.equal(c["past"], torch.cat([padded, got[:, :n]], dim=1)), n
    # before allow-only: text entries are still finite
    assert bool(torch.isfinite(rec.calls[0]["logits"][:, m.vocab.text_tokens[:8]]).all())


def test_returned_tensors_and_errors(small_engine):
    B, steps = 4, 16
    cond = torch.tensor(HP.TAMING_COND).view(-1).cuda()
    q = _gpu_noise(12, steps, B, 16384)
    want = small_engine.generate_hooked(cond, steps, q, HP.hash_bias, 1.0, 250, 0.92)
    # a new fp64 tensor is converted and copied in
    assert torch.equal(small_engine.generate_hooked(cond, steps, q, lambda past_ids, logits: HP.hash_bias(past_ids, logits.clone()).double(),
                                                    1.0, 250, 0.92), want)
    with pytest.raises(ValueError, match="shape"):
        small_engine.generate_hooked(cond, steps, q, lambda past_ids, logits: logits[:, :100], 1.0, 250, 0.92)
    with pytest.raises(TypeError, match="tensor"):
        small_engine.generate_hooked(cond, steps, q, lambda past_ids, logits: None, 1.0, 250, 0.92)
    assert torch.equal(small_engine.generate_hooked(cond, steps, q, HP.hash_bias, 1.0, 250, 0.92), want)


class Boom(Exception):
    pass


@pytest.mark.parametrize("graph", [True, False])
def test_exception_at_step_3_surfaces_and_the_wrapper_stays_usable(graph):
    from wmar_amd.models.taming_wrapper import TamingARMMWrapper
    gcfg, vcfg = synth.GPTConfig(**synth.HARNESS_GPT), synth.VQConfig(**synth.HARNESS_VQ)
    m = TamingARMMWrapper(None, gpt_cfg=gcfg, vq_cfg=vcfg, gpt_state=synth.synth_gpt_state(gcfg, seed=21, logit_scale=40.0),
                          vq_state=synth.synth_vq_state(vcfg, seed=21), max_batch=4)
    m.use_graph = graph
    gp = {"temperature": 1.0, "top_k": 250, "top_p": 0.92}
    q = _gpu_noise(13, 64, 3, 16384)
    want = m.sample([1, 9, 4], gp, q=q, logit_processor=HP.hash_bias)
    err = Boom("at step 3")
    seen = []

    def bad(past_ids, logits):
        seen.append(past_ids.shape[1])
        if past_ids.shape[1] == 4:
            raise err
        return HP.hash_bias(past_ids, logits)

    with pytest.raises(Boom) as e:
        m.sample([1, 9, 4], gp, q=q, logit_processor=bad)
    assert e.value is err and seen == [1, 2, 3, 4]
    assert torch.equal(m.sample([1, 9, 4], gp, q=q, logit_processor=HP.hash_bias), want)
    assert torch.equal(m.sample([1, 9, 4], gp, q=q), m.sample([1, 9, 4], gp, q=q, logit_processor=HP.identity))


# ------------------------------------------------------------------------------------------------- 5. wrapper dispatch
class Foreign:
    """only the reference's interface: spawn_logit_processor / detect / __str__"""

    def __init__(self):
        self.spawned = 0

    def spawn_logit_processor(self):
        self.spawned += 1
        return HP.hash_bias

    def detect(self, codes):
        return torch.full((codes.shape[0],), 0.125, dtype=torch.float64)

    def __str__(self):
        return "foreign-hash"


def _harness_model():
    from wmar_amd.models.taming_wrapper import TamingARMMWrapper
    gcfg, vcfg = synth.GPTConfig(**synth.HARNESS_GPT), synth.VQConfig(**synth.HARNESS_VQ)
    return TamingARMMWrapper(None, gpt_cfg=gcfg, vq_cfg=vcfg, gpt_state=synth.synth_gpt_state(gcfg, seed=21, logit_scale=40.0),
                             vq_state=synth.synth_vq_state(vcfg, seed=21), max_batch=4)


def test_bare_watermarker_runs_through_sample_and_the_harness(tmp_path):
    import json
    from wmar_amd import harness
    m = _harness_model()
    gp = {"batch_size": 4, "temperature": 1.0, "top_k": 250, "top_p": 0.92}
    q = _gpu_noise(14, 64, 6, 16384)       # 6 images on an engine of 4: two chunks
    fw = Foreign()
    m.set_watermarker(fw)
    got = m.sample([1, 9, 4, 1, 9, 4], gp, apply_watermark=True, q=q)
    assert fw.spawned == 1
    assert torch.equal(got, m.sample([1, 9, 4, 1, 9, 4], gp, q=q, logit_processor=HP.hash_bias))     # logit_processor= alone
    assert torch.equal(m.sample([1, 9], gp, apply_watermark=False, q=q[:, :2].contiguous()),
                       m.sample([1, 9], gp, q=q[:, :2].contiguous(), logit_processor=HP.identity))   # apply_watermark=False: no hook
    assert not torch.equal(got[:2], m.sample([1, 9], gp, apply_watermark=False, q=q[:, :2].contiguous()))
    m.set_watermarker(None)
    assert torch.equal(m.sample([1, 9, 4, 1, 9, 4], gp, q=q, logit_processor=HP.hash_bias), got)     # ... and without a watermarker
    # the evaluation harness: generate -> decode -> save -> re-encode -> detect, all through the foreign object
    m.set_watermarker(fw)
    ev = {"metric_names": ["pvalue", "l0", "psnr"], "augmentations": [], "max_roundtrips": 1, "orig_only": False}
    harness.seed_everything(1, 0)
    recs = harness.generate(str(tmp_path), m, [1, 9, 1], fw, ev, gp)
    assert len(recs) > 0
    met = [json.load(open(os.path.join(r, f))) for r, _, fs in os.walk(str(tmp_path)) for f in fs if f.endswith(".json")]
    assert met and all(x["pvalue"] == 0.125 for x in met)
    assert all(r["method"] == "foreign-hash" and r["metrics"]["pvalue"] == 0.125 for r in recs)
    assert all("_foreign-hash_" in f for _, _, fs in os.walk(str(tmp_path)) for f in fs)


def test_gentime_keeps_the_fused_path_and_gumbel_its_own(monkeypatch, kat):
    from wmar_amd.models.engine import GPTEngine, RAREngine
    from wmar_amd.models.rar_wrapper import RarARMMWrapper
    from wmar_amd.watermarking.gumbel_watermark import GumbelWatermark
    calls = []

    def spy(cls, name):
        orig = getattr(cls, name)

        def wrapped(self, *a, **k):
            calls.append(name)
            return orig(self, *a, **k)
        monkeypatch.setattr(cls, name, wrapped)

    for name in ("generate", "generate_hooked"):
        spy(GPTEngine, name)
    for name in ("generate", "generate_hooked", "generate_gumbel", "generate_gumbel_ctx"):
        spy(RAREngine, name)
    m = _harness_model()
    gp = {"temperature": 1.0, "top_k": 250, "top_p": 0.92}
    m.set_watermarker(_wm(kat["keys"]["taming"]))
    m.sample([1, 9], gp, apply_watermark=True)
    assert calls == ["generate"]
    m.sample([1, 9], gp, apply_watermark=True, logit_processor=HP.identity)       # an explicit processor wins
    assert calls == ["generate", "generate_hooked"]
    del calls[:]
    mcfg = synth.MaskgitVQConfig(hidden_channels=32, channel_mult=(1, 2, 2), num_res_blocks=1, resolution=64, z_channels=16,
                                 num_embeddings=1024)
    r = RarARMMWrapper(None, rar_cfg=RCFG, vq_cfg=mcfg, rar_state=synth.synth_rar_state(RCFG, seed=2, logit_scale=30.0),
                       vq_state=synth.synth_maskgit_state(mcfg, seed=4), max_batch=4)
    r.set_watermarker(GumbelWatermark(1024, seed=42, device="cuda", ngram=0))
    r.sample([3, 7], None, apply_watermark=True)
    r.set_watermarker(GumbelWatermark(1024, seed=42, device="cuda", ngram=2))
    r.sample([3, 7], None, apply_watermark=True)
    r.set_watermarker(_wm(kat["keys"]["rar"]))
    r.sample([3, 7], None, apply_watermark=True)
    r.set_watermarker(Foreign())
    r.sample([3, 7], None, apply_watermark=True)
    assert calls == ["generate_gumbel", "generate_gumbel_ctx", "generate", "generate_hooked"]


def test_sample_interleaved_image_phases_honour_the_hook():
    from wmar_amd.models.chameleon_wrapper import ChameleonARMMWrapper
    from wmar_amd.watermarking.gentime_watermark import GentimeWatermark, SeedStrategy, SplitStrategy
    cfg = synth.ChameleonConfig(dim=256, n_layers=2, n_heads=4, n_kv_heads=4, vocab_size=2048, multiple_of=64)
    vq_cfg = synth.VQConfig(ch=32, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(), resolution=16, z_channels=32, embed_dim=32,
                            n_embed=512)
    m = ChameleonARMMWrapper(None, 0, cfg=cfg, state=synth.synth_chameleon_state(cfg, seed=8, logit_scale=6.0),
                             vocab_map=synth.synth_chameleon_vocab(2048, 512), vq_cfg=vq_cfg, vq_state=synth.synth_vq_state(vq_cfg, 1),
                             max_batch=2, max_prompt_len=80)           # max_seq_len 80 + 64: room for two images
    v = m.vocab
    m._allow_text = torch.tensor([v.begin_image], dtype=torch.int64, device="cuda")       # every text step hands over to the image decoder
    wm = GentimeWatermark(m.get_vq(), 2048, SeedStrategy.LINEAR, SplitStrategy.RANDOM_STRATIFIED, 1, 3.0, 0.25, device="cuda")
    gp = {"temperature": 0.9, "top_p": 0.8}
    p = [v.text_tokens[3], v.text_tokens[50]]

    def run(**kw):
        m.seed = 2
        return [(k, t.cpu().tolist()) for k, t in m.sample_interleaved([(0, p)], gp, max_gen_len=140, **kw)]

    m.set_watermarker(wm, None)
    fused = run(apply_watermark=True)
    images = [t for k, t in fused if k == "image_seg"]
    assert len(images) >= 2
    m.set_watermarker(None, None)
    assert run(logit_processor=HP.greenlist_from_table(wm)) == fused
    banned = [t for k, t in run(logit_processor=HP.ban_repeats) if k == "image_seg"]
    first = [tok for t in banned[:4] for tok in t[0]]          # (c) sees the whole growing input row: no image token twice, within an
    assert len(banned) >= 2 and len(set(first)) == len(first)  # image or across images (at most 4 x 64 of the 512 image tokens)


# --------------------------------------------------------------------------------------------------- 6. re-run and reuse
_CHILD_RERUN = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
from tests import hook_processors as HP
from wmar_amd.utils import synth
from wmar_amd.models.engine import GPTEngine
cfg = synth.GPTConfig(vocab_size=16384, block_size=16, n_layer=2, n_head=24, n_embd=1536)
eng = GPTEngine(cfg, synth.synth_gpt_state_fast(cfg, seed=1, device="cuda", logit_scale=10.0), max_batch=64)
print("PLAN0", eng.plan_info(64)["proj"])
q = torch.empty(16, 64, cfg.vocab_size, device="cuda").exponential_(1, generator=torch.Generator(device="cuda").manual_seed(7))
cond = torch.arange(64).cuda()
first = []
def proc(past_ids, logits):
    if past_ids.shape[1] == 1:
        first.append(1)
    return HP.hash_bias(past_ids, logits)
hurt = eng.generate_hooked(cond, 16, q, proc, 1.0, 250, 0.92)
print("STEP0_CALLS", len(first))
info = eng.plan_info(64)
print("PLAN1", info["proj"])
print("FALLBACKS", info["barrier_fallbacks"])
del first[:]
clean = eng.generate_hooked(cond, 16, q, proc, 1.0, 250, 0.92)
print("STEP0_CALLS_CLEAN", len(first))
print("FALLBACKS2", eng.plan_info(64)["barrier_fallbacks"])
np.savez(sys.argv[1], hurt=hurt.cpu().numpy(), clean=clean.cpu().numpy())
"""


def test_failed_barrier_reruns_the_hooked_generation_from_step_0(tmp_path):
    """WMAR_INJECT_SYNC_FAIL=1 at 64 rows: the flag is found behind the last step, the engine switches to the two-launch path and the
    run is repeated -- the processor sees step 0 twice, the caller gets the tokens of a clean run"""
    out = tmp_path / "rerun.npz"
    res = subprocess.run([sys.executable, "-c", _CHILD_RERUN % REPO, str(out)], env=dict(os.environ, WMAR_INJECT_SYNC_FAIL="1"),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    tags = {l.split()[0]: l.split(None, 1)[1] for l in res.stdout.splitlines() if l.split() and l.split()[0].isupper()}
    assert "k_bx_xr" in tags["PLAN0"] and "k_bx<1" in tags["PLAN1"], tags
    assert tags["STEP0_CALLS"] == "2" and tags["FALLBACKS"] == "1" and tags["STEP0_CALLS_CLEAN"] == "1" and tags["FALLBACKS2"] == "1", tags
    z = np.load(out)
    assert np.array_equal(z["hurt"], z["clean"])


def test_alternating_fused_and_hooked_calls_stay_equal(prod_engine, wm_taming):
    """fused and hooked graphs live in slots of their own; five alternations, then eager: the same tokens every time"""
    wm, green = wm_taming
    cond = torch.arange(64).cuda()
    q = _gpu_noise(15, 16, 64, 16384)
    first = prod_engine.generate(cond, 16, q, 1.0, 250, 0.92, wm.wm_ctx()).clone()
    for rep in range(5):
        assert torch.equal(prod_engine.generate_hooked(cond, 16, q, green, 1.0, 250, 0.92), first), f"hooked replay {rep + 1}"
        assert torch.equal(prod_engine.generate(cond, 16, q, 1.0, 250, 0.92, wm.wm_ctx()), first), f"fused replay {rep + 1}"
    assert torch.equal(prod_engine.generate_hooked(cond, 16, q, green, 1.0, 250, 0.92, use_graph=False), first)
