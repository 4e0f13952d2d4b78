"""Chameleon engine against the CPU oracle at the shapes the benchmark runs and at the decompositions the small fixtures of
test_gpu_chameleon.py never reach: widths whose stream-K GEMMs split a column group across workgroups, 1K-token caches (many
attention chunks on both waves, RoPE past position 1000), the 7B width at 3 / 48 / 126 rows, all 32 layers of the 7B model and
the captured loop at 1024 image tokens.

Gates are test_gpu_chameleon.py::_close's: 3 % of the logit standard deviation against `fold=True` (the engine's algebra), 8 %
against `fold=False` (the reference's rounding points), each plus one bf16 ulp of the largest logit; 4x the first for 32 layers.
Rows are independent in the engine, so the engine runs every row and the oracle checks a subset holding a row of each 32-row
tile and the last row.  Every leg prints its measured max |dlogit| / std, arg-max agreement and timings."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cham_oracle as CO  # noqa: E402
from tests.test_gpu_chameleon import _close, replay_oracle_chain  # noqa: E402
from wmar_amd.utils import synth  # noqa: E402

# ------------------------------------------------------------------ stream-K decomposition, restated from cham.hip / cham_kernels.h
BG_TG, BG_KC, BG_MAXP, GRID = 4, 8, 16, 256


def _wg_of(k, u):
    C, U, G = k
    return ((u + 1) * G - 1) // U


def _count(k, g):                      # sk_count: pieces of column group g
    C = k[0]
    return _wg_of(k, g * C + C - 1) - _wg_of(k, g * C) + 1


def _sk_for(NT, KB, whole_groups):     # sk_for (cham.hip): (chunks per group, units, workgroups)
    groups = -(-NT // BG_TG)
    C = -(-KB // BG_KC)
    U = groups * C
    if whole_groups:
        per = -(-groups // GRID)
        while groups % per:
            per += 1
        return C, U, groups // per
    G = min(GRID, U)
    while G > 1 and max(_count((C, U, G), g) for g in range(groups)) > BG_MAXP:
        G -= 16 if G > 64 else 1
    return C, U, G


def decomposition(cfg):
    """Which stream-K cases the five GEMMs of `cfg` reach (ChamPlan's sk_qkv / sk_o / sk_13 / sk_2 / sk_head)."""
    D, Dkv, F = cfg.dim, cfg.n_kv_heads * cfg.head_dim, cfg.ffn_hidden
    gemms = {"qkv": ((D + 2 * Dkv) // 32, D // 16, False), "o": (D // 32, D // 16, False), "w13": (F // 16, D // 16, False),
             "w2": (D // 32, F // 16, False), "head": (cfg.vocab_size // 32, D // 16, True)}
    cases = set()
    for name, (NT, KB, whole) in gemms.items():
        k = _sk_for(NT, KB, whole)
        C, U, G = k
        groups = -(-NT // BG_TG)
        maxp = max(_count(k, g) for g in range(groups))
        assert maxp <= BG_MAXP
        if name == "qkv" and maxp > 4:
            cases.add("attention prologue > 4 pieces")
        if not whole and maxp == BG_MAXP:
            cases.add("BG_MAXP pieces")
        if not whole and G < min(GRID, U):
            cases.add("grid cut by BG_MAXP")
        if not whole and any(len({u // C for u in range(w * U // G, (w + 1) * U // G)}) > 1 for w in range(G)):
            cases.add("workgroup boundary inside a group")
        if not whole and NT % BG_TG:
            cases.add("NT % 4 != 0")
        if KB % BG_KC:
            cases.add("partial last K chunk")
        if whole and NT % BG_TG:
            cases.add("partial last head group")
        if whole and groups // G > 1:
            cases.add("head: several groups per workgroup")
    return cases


# (dim, heads, kv heads, vocab, multiple_of) -> the cases the sweep claims for it
SWEEP = {
    (1024, 8, 8, 1024, 64): {"attention prologue > 4 pieces", "BG_MAXP pieces", "grid cut by BG_MAXP", "workgroup boundary inside a group",
                             "partial last K chunk"},
    (2048, 16, 16, 1024, 64): {"attention prologue > 4 pieces", "BG_MAXP pieces", "workgroup boundary inside a group"},
    (1536, 12, 4, 2080, 64): {"attention prologue > 4 pieces", "BG_MAXP pieces", "grid cut by BG_MAXP", "partial last head group"},
    (320, 5, 1, 1056, 16): {"NT % 4 != 0", "partial last K chunk", "partial last head group"},
}
ALL_CASES = {"attention prologue > 4 pieces", "BG_MAXP pieces", "grid cut by BG_MAXP", "workgroup boundary inside a group", "NT % 4 != 0",
             "partial last K chunk", "partial last head group"}


def _cham_cfg(dim, heads, kv, vocab, multiple_of=64, layers=2, qk=True):
    return synth.ChameleonConfig(dim=dim, n_layers=layers, n_heads=heads, n_kv_heads=kv, vocab_size=vocab, multiple_of=multiple_of,
                                 qk_normalization=qk)


def test_sweep_covers_every_decomposition():
    """The restatement agrees with the tested shapes' known decomposition and the sweep (plus the 7B leg) reaches every case."""
    assert decomposition(_cham_cfg(256, 4, 4, 1024)) == {"partial last K chunk"}          # test_gpu_chameleon.py's widths: FC2 K only
    assert decomposition(_cham_cfg(512, 4, 4, 1024)) == set()
    seen = set()
    for shape, claimed in SWEEP.items():
        got = decomposition(_cham_cfg(*shape))
        assert claimed <= got, (shape, claimed - got)
        seen |= got
    assert ALL_CASES <= seen, ALL_CASES - seen
    assert {"workgroup boundary inside a group", "head: several groups per workgroup"} <= decomposition(synth.ChameleonConfig(n_layers=2))


def _subset(M):
    """oracle rows: one per 32-row tile (spread inside the tiles) and the last row"""
    return sorted({min(32 * t + (7 * t) % 32, M - 1) for t in range((M + 31) // 32)} | {M - 1})


def _report(tag, got, ref, frac):
    err, scale = float((got - ref).abs().max()), float(ref.std())
    am = (got.argmax(-1) == ref.argmax(-1)).float().mean()
    print(f"  {tag}: max |dlogit| {err:.4f} = {err / scale:.4f} std (gate {frac} std + 1 ulp), arg-max agree {float(am) * 100:.1f} %")
    _close(got, ref, frac)
    return err / scale


# ------------------------------------------------------------------------------------------------------ a. stream-K sweep
@pytest.mark.parametrize("max_batch", [10, 42])           # 30 rows (one tile) and 126 rows (four tiles)
@pytest.mark.parametrize("shape", list(SWEEP), ids=lambda s: f"d{s[0]}h{s[1]}kv{s[2]}v{s[3]}")
def test_streamk_shapes_vs_oracle(shape, max_batch):
    from wmar_amd.models.engine import ChameleonEngine
    cfg = _cham_cfg(*shape)
    sd = synth.synth_chameleon_state(cfg, seed=sum(shape), logit_scale=4.0)
    M = 3 * max_batch
    e = ChameleonEngine(cfg, sd, max_batch=max_batch, max_seq_len=16)
    rows = _subset(M)
    rs = np.random.RandomState(M + shape[0])
    cache_f, cache_r = CO.Cache(cfg.n_layers, len(rows)), CO.Cache(cfg.n_layers, len(rows))
    start = torch.from_numpy(rs.randint(0, 3, size=M).astype(np.int32))      # right-aligned: a row idles at position 0 until it starts
    t0 = time.perf_counter()
    print(f"\nstream-K {shape} x {M} rows (oracle rows {rows}): {sorted(decomposition(cfg))}")
    for step in range(6):
        tok = torch.from_numpy(rs.randint(0, cfg.vocab_size, size=M).astype(np.int64))
        pos = torch.clamp(step - start, min=0).to(torch.int32)
        got = e.forward_tokens(tok.cuda(), pos.cuda()).cpu()[rows]
        ref_f = CO.forward_tokens(sd, cfg, tok[rows], pos[rows], cache_f, fold=True)
        ref_r = CO.forward_tokens(sd, cfg, tok[rows], pos[rows], cache_r, fold=False)
        _report(f"step {step} fold=True ", got, ref_f, 0.03)
        _report(f"step {step} fold=False", got, ref_r, 0.08)
    print(f"  {time.perf_counter() - t0:.1f} s")


# ------------------------------------------------------------------------------------------------------ b. long caches
@pytest.mark.parametrize("dim,kv", [(512, 4), (512, 1), (256, 4), (256, 1)])
def test_long_cache_vs_prefix(dim, kv):
    """1107-row caches (not a multiple of the 16- / 32-row attention chunk), rows started at different steps (right-aligned
    prompts), logits on both sides of every chunk edge and loop edge (4 chunks per trip of the two-wave loop), past 1024 and at
    the last cache row; RoPE up to position 1106."""
    from wmar_amd.models.engine import ChameleonEngine
    cfg = _cham_cfg(dim, 4, kv, 1024)
    hd = cfg.head_dim
    sd = synth.synth_chameleon_state(cfg, seed=dim + kv, logit_scale=4.0)
    Tmax, offsets = 1107, [0, 1, 2, 5, 16, 33]
    R = len(offsets)
    e = ChameleonEngine(cfg, sd, max_batch=2, max_seq_len=Tmax)
    E = 16 if hd == 128 else 32                                   # cached rows per attention chunk
    lengths = sorted({1, 2, E, E + 1, 2 * E, 2 * E + 1, 4 * E, 4 * E + 1, 8 * E, 8 * E + 1, 1024, 1025, Tmax})
    check = [L - 1 for L in lengths]                               # position P sees a cache of P + 1 rows
    rs = np.random.RandomState(dim * 10 + kv)
    seq = torch.from_numpy(rs.randint(0, cfg.vocab_size, size=(R, Tmax)).astype(np.int64))
    seq_d = seq.cuda()
    off = torch.tensor(offsets, dtype=torch.int32)
    got = {}
    t0 = time.perf_counter()
    for j in range(Tmax):
        pos = torch.clamp(j - off, min=0)
        live = j >= off
        want = any(bool(live[r]) and int(pos[r]) in check for r in range(R))
        tok = torch.where(live.cuda(), seq_d[torch.arange(R, device="cuda"), pos.cuda().long()], torch.zeros_like(seq_d[:, 0]))
        lg = e.forward_tokens(tok, pos.cuda(), want_logits=want)
        if want:
            lg = lg.cpu()
            for r in range(R):
                if live[r] and int(pos[r]) in check:
                    got[(r, int(pos[r]))] = lg[r]
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = {f: CO.prefix(sd, cfg, seq, check, fold=f) for f in (True, False)}
    t_cpu = time.perf_counter() - t0
    print(f"\nlong cache dim {dim} hd {hd} kv {kv}: {Tmax} steps x {R} rows (offsets {offsets}), engine {t_gpu:.1f} s, prefix {t_cpu:.1f} s")
    worst = {True: 0.0, False: 0.0}
    for i, P in enumerate(check):
        rr = [r for r in range(R) if (r, P) in got]
        g = torch.stack([got[(r, P)] for r in rr])
        for f, frac in ((True, 0.03), (False, 0.08)):
            rf = ref[f][rr, i]
            err = float((g - rf).abs().max()) / float(rf.std())
            worst[f] = max(worst[f], err)
            _close(g, rf, frac)
    print(f"  cache lengths {lengths}: worst max |dlogit| / std {worst[True]:.4f} (fold=True), {worst[False]:.4f} (fold=False)")


# ------------------------------------------------------------------------------------------------------ c. 7B width, 2 layers
@pytest.fixture(scope="module")
def cham7b_2l():
    cfg = synth.ChameleonConfig(n_layers=2)
    assert (cfg.dim, cfg.n_heads, cfg.head_dim, cfg.ffn_hidden, cfg.vocab_size) == (4096, 32, 128, 11008, 65536)
    t0 = time.perf_counter()
    sd_dev = synth.synth_chameleon_state(cfg, seed=7, device="cuda", logit_scale=4.0, gen_device="cuda")
    sd = {k: v.to("cpu", torch.float32) for k, v in sd_dev.items()}      # 3.8 GB: the incremental oracle converts no weights per step
    print(f"\n7B x 2 layers: weights generated and copied in {time.perf_counter() - t0:.1f} s")
    yield cfg, sd_dev, sd
    del sd_dev
    torch.cuda.empty_cache()


def test_7b_width_48_rows_long_and_resize(cham7b_2l):
    """The bench's plan (48 rows, two row tiles) teacher-forced to position 1040, against one prefix pass; then the live engine
    shrunk to 5 rows restarting at position 0 and grown back to 48 (rows 5.. continue their 1041-token sequences)."""
    from wmar_amd.models.engine import ChameleonEngine
    cfg, sd_dev, sd = cham7b_2l
    M, Tn = 48, 1041
    check = [0, 1, 16, 17, 1023, 1024, Tn - 1]
    rows = _subset(M)
    e = ChameleonEngine(cfg, sd_dev, max_batch=16)
    rs = np.random.RandomState(4096)
    seq = torch.from_numpy(rs.randint(0, cfg.vocab_size, size=(M, Tn + 1)).astype(np.int64))
    seq_d = seq.cuda()
    got = {}
    t0 = time.perf_counter()
    for t in range(Tn):
        lg = e.forward_tokens(seq_d[:, t], torch.full((M,), t, dtype=torch.int32, device="cuda"), want_logits=t in check)
        if t in check:
            got[t] = lg[rows].cpu()
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = {f: CO.prefix(sd, cfg, seq[rows], check + [Tn], fold=f) for f in (True, False)}
    t_cpu = time.perf_counter() - t0
    print(f"\n7B width, 48 rows to position {Tn - 1} (oracle rows {rows}): engine {t_gpu:.1f} s, prefix x 2 {t_cpu:.1f} s")
    for i, t in enumerate(check):
        _report(f"position {t:4d} fold=True ", got[t], ref[True][:, i], 0.03)
        _report(f"position {t:4d} fold=False", got[t], ref[False][:, i], 0.08)
    # shrink: 5 rows restart at position 0
    small = 5
    cache = CO.Cache(cfg.n_layers, small)
    for t in range(3):
        tok = torch.from_numpy(rs.randint(0, cfg.vocab_size, size=small).astype(np.int64))
        pos = torch.full((small,), t, dtype=torch.int32)
        g = e.forward_tokens(tok.cuda(), pos.cuda()).cpu()
        _report(f"shrunk to {small} rows, position {t}", g, CO.forward_tokens(sd, cfg, tok, pos, cache, fold=True), 0.03)
    # grow back: rows 0..4 continue at position 3, rows 5..47 continue at position 1041 (their caches untouched by the 5-row steps)
    tok = seq[:, Tn].clone()
    tok[:small] = torch.from_numpy(rs.randint(0, cfg.vocab_size, size=small).astype(np.int64))
    pos = torch.full((M,), Tn, dtype=torch.int32)
    pos[:small] = 3
    g = e.forward_tokens(tok.cuda(), pos.cuda()).cpu()
    _report("grown to 48, rows 0..4 at position 3", g[:small], CO.forward_tokens(sd, cfg, tok[:small], pos[:small], cache, fold=True), 0.03)
    far = [r for r in rows if r >= small]
    _report(f"grown to 48, rows {far} at position {Tn}", g[far], ref[True][[rows.index(r) for r in far], len(check)], 0.03)


@pytest.mark.parametrize("M", [3, 126])
def test_7b_width_short_runs_both_folds(cham7b_2l, M):
    from wmar_amd.models.engine import ChameleonEngine
    cfg, sd_dev, sd = cham7b_2l
    e = ChameleonEngine(cfg, sd_dev, max_batch=M // 3, max_seq_len=16)
    rows = _subset(M)
    rs = np.random.RandomState(M)
    cache_f, cache_r = CO.Cache(cfg.n_layers, len(rows)), CO.Cache(cfg.n_layers, len(rows))
    t0 = time.perf_counter()
    print(f"\n7B width, {M} rows (oracle rows {rows}):")
    for t in range(3):
        tok = torch.from_numpy(rs.randint(0, cfg.vocab_size, size=M).astype(np.int64))
        pos = torch.full((M,), t, dtype=torch.int32)
        got = e.forward_tokens(tok.cuda(), pos.cuda()).cpu()[rows]
        _report(f"position {t} fold=True ", got, CO.forward_tokens(sd, cfg, tok[rows], pos[rows], cache_f, fold=True), 0.03)
        _report(f"position {t} fold=False", got, CO.forward_tokens(sd, cfg, tok[rows], pos[rows], cache_r, fold=False), 0.08)
    print(f"  {time.perf_counter() - t0:.1f} s")
    del e


# ------------------------------------------------------------------------------------------------------ d. 32 layers at 7B
def test_7b_32_layers_vs_prefix():
    """CHAMELEON_7B (all 32 blocks: the weight-pack offsets of layers >= 2, the bf16 error over 32 residual blocks), 48 rows.
    The host copy stays bf16 (13.5 GB); the oracle converts one weight at a time.  Gate: 4x the 2-layer fold=True gate (the rule of
    test_gpu_depth.py); an arg-max may move only between logits closer than that gate.  fold=False is reported."""
    from wmar_amd.models.engine import ChameleonEngine
    cfg = synth.CHAMELEON_7B
    assert cfg.n_layers == 32
    t0 = time.perf_counter()
    sd_dev = synth.synth_chameleon_state(cfg, seed=32, device="cuda", logit_scale=4.0, gen_device="cuda")
    e = ChameleonEngine(cfg, sd_dev, max_batch=16, max_seq_len=64)
    sd = {k: v.to("cpu") for k, v in sd_dev.items()}
    del sd_dev
    torch.cuda.empty_cache()
    t_setup = time.perf_counter() - t0
    M, Tn = 48, 40
    check = [0, 1, 17, Tn - 1]
    rows = _subset(M)
    rs = np.random.RandomState(32)
    seq = torch.from_numpy(rs.randint(0, cfg.vocab_size, size=(M, Tn)).astype(np.int64))
    seq_d = seq.cuda()
    got = {}
    for t in range(Tn):
        lg = e.forward_tokens(seq_d[:, t], torch.full((M,), t, dtype=torch.int32, device="cuda"), want_logits=t in check)
        if t in check:
            got[t] = lg[rows].cpu()
    t0 = time.perf_counter()
    ref = {f: CO.prefix(sd, cfg, seq[rows], check, fold=f) for f in (True, False)}
    t_cpu = time.perf_counter() - t0
    print(f"\n7B x 32 layers, 48 rows (oracle rows {rows}): setup {t_setup:.1f} s, prefix x 2 {t_cpu:.1f} s")
    gate = 4 * 0.03
    for i, t in enumerate(check):
        g, rf, rr = got[t], ref[True][:, i], ref[False][:, i]
        err, scale = float((g - rf).abs().max()), float(rf.std())
        errr = float((g - rr).abs().max()) / float(rr.std())
        print(f"  position {t:2d}: max |dlogit| {err / scale:.4f} std (fold=True, gate {gate}), {errr:.4f} std (fold=False)")
        _close(g, rf, gate)
        am, ram = g.argmax(-1), rf.argmax(-1)
        for b in np.nonzero((am != ram).numpy())[0]:
            assert float(rf[b, ram[b]] - rf[b, am[b]]) < gate * scale + 2.0 ** -7 * float(rf.abs().max()), (t, b)
    del e


# ------------------------------------------------------------------------------------------------------ e. the captured loop at 1024 tokens
def test_generate_image_loop_1024_tokens():
    """test_gpu_chameleon.py::test_generate_image_loop's oracle chain at the production token count: the loop's position and
    watermark-context tables over 1024 steps (captured graph, linear watermark, top-p)."""
    from wmar_amd.models.chameleon_wrapper import ChameleonARMMWrapper
    from wmar_amd.watermarking.gentime_watermark import GentimeWatermark, SeedStrategy, SplitStrategy
    cfg = _cham_cfg(256, 4, 4, 2048)
    vq_cfg = synth.VQConfig(ch=32, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(), resolution=16, z_channels=32, embed_dim=32,
                            n_embed=512)
    sd = synth.synth_chameleon_state(cfg, seed=8, logit_scale=6.0)
    m = ChameleonARMMWrapper(None, 0, cfg=cfg, state=sd, vocab_map=synth.synth_chameleon_vocab(2048, 512), vq_cfg=vq_cfg,
                             vq_state=synth.synth_vq_state(vq_cfg, 1), max_batch=3, max_prompt_len=16)
    m.n_image_tokens = 1024                      # the engine was sized for 16 + 1024 positions (the class default)
    m.is_codes_shaped = lambda c: True
    m.use_graph = True
    wm = GentimeWatermark(m.get_vq(), 2048, SeedStrategy.LINEAR, SplitStrategy.RANDOM_STRATIFIED, 1, 3.0, 0.25, device="cuda")
    m.set_watermarker(wm)
    text = m.vocab.text_tokens
    cond = [(0, [text[5], text[9], text[100]]), (1, [text[7]]), (2, [text[1], text[2], text[3], text[4], text[400]])]
    torch.manual_seed(3)
    q = m.draw_noise(3)
    t0 = time.perf_counter()
    codes = m.sample(cond, {"temperature": 0.9, "top_p": 0.8}, apply_watermark=True, q=q)
    assert codes.shape == (3, 1024) and set(codes.flatten().tolist()) <= set(m.vocab.image_tokens)
    t_loop = time.perf_counter() - t0
    t0 = time.perf_counter()
    replay_oracle_chain(m, wm, cfg, sd, cond, q, codes, 1, 1024)
    print(f"\ncaptured loop, 1024 tokens x 3 images: loop {t_loop:.2f} s, replay + oracle chain {time.perf_counter() - t0:.1f} s")
