"""Context-keyed Gumbel watermark (ngram > 0): key rows derived on the device, keyed generation inside the captured RAR step and the
first-occurrence detector, against the host key builder and the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import rar_oracle as R  # noqa: E402
from oracle import wm_oracle as W  # noqa: E402
from wmar_amd.utils import synth  # noqa: E402


def _h0(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return int(torch.randint(0, 2 ** 31 - 1, (1,), generator=g).item())


def _host_key(h, V):
    from wmar_amd import _lib
    rs, lr, sc = (np.zeros(V, np.float32) for _ in range(3))
    _lib.check(_lib.load().wmar_gumbel_key_build(C.c_uint64(int(h) & 0xFFFFFFFFFFFFFFFF), V, rs.ctypes.data, lr.ctypes.data,
                                                  sc.ctypes.data))
    return rs, lr, sc


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ (a) key rows
def _edge_hashes(n, seed):
    rs = np.random.RandomState(seed)
    h = rs.randint(0, 2 ** 31 - 1, size=n).astype(np.int64)
    edge = [0, 2 ** 31 - 2, 2 ** 32 + 5, 2 ** 40 + 123456789, (2 ** 63 - 1), -1, -2 ** 63, -123456789012345, 2 ** 32, 1]
    h[:len(edge)] = np.array(edge, dtype=np.int64)
    assert len(set(h.tolist())) == n      # distinct as int64 (2^32 and 0 share their low word on purpose)
    return h


def test_key_rows_bit_equal_to_host_builder_4096_hashes_at_16384():
    """67 M entries of each array (about 98 % of the 2^24 possible rs values): zero mismatches, no tolerance."""
    from wmar_amd.watermarking.gumbel_watermark import key_rows
    V, N = 16384, 4096
    h = _edge_hashes(N, 7)
    bad = [0, 0, 0]
    for c0 in range(0, N, 512):       # 512 x 16384 x 3 arrays = 100 MB per pass
        got = [t.cpu().numpy() for t in key_rows(torch.from_numpy(h[c0:c0 + 512]), V, "cuda")]
        for i in range(512):
            ref = _host_key(h[c0 + i], V)
            for k in range(3):
                if not _same_bits(got[k][i], ref[k]):
                    bad[k] += int((got[k][i].view(np.uint32) != ref[k].view(np.uint32)).sum())
    print("mismatching entries (rs, log_rs, score):", bad)
    assert bad == [0, 0, 0]


@pytest.mark.parametrize("V", [1, 37, 623, 624, 625, 1024])
def test_key_rows_block_edges(V):
    from wmar_amd.watermarking.gumbel_watermark import key_rows
    h = _edge_hashes(64, V)
    got = [t.cpu().numpy() for t in key_rows(torch.from_numpy(h).cuda(), V, "cuda")]
    for i in range(64):
        ref = _host_key(h[i], V)
        for k in range(3):
            assert _same_bits(got[k][i], ref[k]), (V, i, k)
    only = key_rows(torch.from_numpy(h), V, "cuda", want=(False, True, False))
    assert only[0] is None and only[2] is None and torch.equal(only[1].cpu(), torch.from_numpy(got[1]))


# ------------------------------------------------------------------ (b) eager sampler / score with per-row hashes
@pytest.mark.parametrize("V,B", [(1024, 64), (16384, 5), (1000, 3), (37, 2)])
def test_gumbel_sample_distinct_hashes_without_host_builds(V, B, monkeypatch):
    from wmar_amd import _lib
    from wmar_amd.watermarking import gumbel_watermark as G
    rs = np.random.RandomState(V + B)
    lg = (rs.randn(B, V) * 4).astype(np.float32)
    lg[0, : V // 2] = lg[0, 0]
    h = torch.from_numpy(rs.randint(0, 2 ** 31, size=B).astype(np.int64))
    if B == 64:
        h[3], h[9] = -5, 2 ** 35 + 17
    assert len(set(h.tolist())) == B
    calls = []
    real = _lib.load()

    class Spy:
        def __getattr__(self, name):
            if name == "wmar_gumbel_key_build":
                calls.append(name)
            return getattr(real, name)

    monkeypatch.setattr(G._lib, "load", lambda: Spy())
    toks = torch.from_numpy(rs.randint(0, V, size=B).astype(np.int64)).cuda()
    for temp, top_p, top_k in [(1.0, 0.0, 0), (0.6, 0.0, 0), (1.0, 0.3, 0), (1.3, 0.95, 0), (1.0, 1.0, 0), (1.0, 0.0, 7),
                               (0.9, 0.0, 10 ** 6)]:
        got = G.gumbel_sample(torch.from_numpy(lg).cuda(), h, True, temp, top_p, top_k).cpu().numpy()
        assert np.array_equal(got, W.gumbel_sample(lg, h.numpy(), True, temp, top_p, top_k)), (temp, top_p, top_k)
    sc = G.gumbel_score_tok(toks, h.cuda(), V)          # hashes already on the device: never read back
    assert np.array_equal(sc.cpu().numpy(), W.gumbel_score_tok(toks.cpu().numpy(), h.numpy(), V))
    assert calls == [], "per-row hashes went through the host key builder"


# ------------------------------------------------------------------ (c) keyed generation
def _oracle_ctx_sampler(seed, n, u, V, temp, top_p, top_k):
    """sampler(mixed logits, step) of oracle.rar_oracle.generate: unkeyed below n (the key row is u[step, b]), else keyed by
    h0 ^ the n ids in front.  Keeps the tokens it returned."""
    h0, hist = _h0(seed), []

    def f(mixed, step):
        lg = np.ascontiguousarray(mixed.numpy().astype(np.float32))
        B = lg.shape[0]
        if step < n:
            tok = np.array([W.lib().wmo_gumbel_sample_row(np.ascontiguousarray(lg[b]), V, np.ascontiguousarray(u[step, b]), 1,
                                                          float(temp), float(top_p), int(top_k)) for b in range(B)], dtype=np.int64)
        else:
            hs = np.full(B, h0, dtype=np.int64)
            for i in range(n):
                hs ^= hist[step - n + i]
            tok = W.gumbel_sample(lg, hs, True, temp, top_p, top_k)
        hist.append(tok.copy())
        return torch.from_numpy(tok)

    return f


SMALL = synth.RARConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, image_seq_len=64,
                        codebook_size=256, condition_num_classes=1000)
SMALL_VQ = synth.MaskgitVQConfig(hidden_channels=32, channel_mult=(1, 2, 2), num_res_blocks=1, resolution=32, z_channels=16,
                                 num_embeddings=256)


@pytest.fixture(scope="module")
def small():
    from wmar_amd.models.rar_wrapper import RarARMMWrapper
    rsd = synth.synth_rar_state(SMALL, seed=1, logit_scale=6.0)
    m = RarARMMWrapper(None, rar_cfg=SMALL, vq_cfg=SMALL_VQ, rar_state=rsd, vq_state=synth.synth_maskgit_state(SMALL_VQ, seed=1),
                       max_batch=4)
    return m, rsd


def _keyed(m, cond, wm, seed, graph=True):
    m.set_watermarker(wm)
    m.use_graph = graph
    torch.manual_seed(seed)
    u = m.draw_gumbel_noise(len(cond), wm.ngram)
    return m.sample(cond, None, apply_watermark=True, q=u), u


@pytest.mark.parametrize("ngram,top_p,top_k", [(1, 0.0, 0), (2, 0.0, 0), (4, 0.0, 0), (2, 0.9, 0), (1, 0.0, 50)])
def test_rar_generate_gumbel_ctx_vs_oracle(small, ngram, top_p, top_k):
    """Guidance on, graph and eager: tokens equal the step-by-step oracle fed the same u.  Six classes over max_batch 4: two chunks."""
    from wmar_amd.watermarking.gumbel_watermark import GumbelWatermark
    m, rsd = small
    wm = GumbelWatermark(256, seed=1234, temperature=1.0, top_p=top_p, top_k=top_k, device="cuda", ngram=ngram)
    cond = torch.tensor([3, 500, 77, 9, 12, 999])
    ref = None
    for graph in (True, False):
        codes, u = _keyed(m, cond, wm, 11, graph)
        if ref is None:
            ref = R.generate(rsd, SMALL, cond, 4.0, 0.0, 1.0, None, 0.0, draw_drop_mask=False,
                             sampler=_oracle_ctx_sampler(1234, ngram, u.cpu().numpy(), 256, 1.0, top_p, top_k))
        assert torch.equal(codes.cpu(), ref), (graph, [int((c != r).nonzero()[0]) if (c != r).any() else -1
                                                       for c, r in zip(codes.cpu(), ref)])
    # the wrapper's own draws: the label-drop mask [B, 1], then ngram tensors [B, V] per chunk of max_batch rows
    torch.manual_seed(11)
    mine = m.sample(cond, None, apply_watermark=True)
    torch.manual_seed(11)
    us = [m.draw_gumbel_noise(4, ngram), m.draw_gumbel_noise(2, ngram)]
    assert torch.equal(mine, m.sample(cond, None, apply_watermark=True, q=torch.cat(us, dim=1)))


def test_rar_xl_width_128_rows_gumbel_ctx_vs_oracle():
    """RAR-XL width, 2 layers, batch 64 under guidance (128 rows, the bf16-piece GEMM path), 256 positions, ngram = 1."""
    from wmar_amd.models.engine import RAREngine
    cfg = synth.RARConfig(hidden_size=1280, num_hidden_layers=2, num_attention_heads=16, intermediate_size=5120, image_seq_len=256,
                          codebook_size=1024, condition_num_classes=1000)
    rsd = synth.synth_rar_state(cfg, seed=12, logit_scale=8.0)
    eng = RAREngine(cfg, rsd, max_batch=64)
    cond = torch.arange(64) * 13 % 1000
    u = torch.rand(1, 64, 1024, generator=torch.Generator().manual_seed(4))
    got = eng.generate_gumbel_ctx(cond.cuda(), _h0(99), 1, u.cuda(), R.cfg_scales(256, 4.0, 0.0), 1.0, 0.0, 0)
    ref = R.generate(rsd, cfg, cond, 4.0, 0.0, 1.0, None, 0.0, draw_drop_mask=False,
                     sampler=_oracle_ctx_sampler(99, 1, u.numpy(), 1024, 1.0, 0.0, 0))
    got = got.cpu()
    assert torch.equal(got, ref), f"first mismatch per row: {[(int((g != r).nonzero()[0]) if (g != r).any() else -1) for g, r in zip(got, ref)]}"


# ------------------------------------------------------------------ (d) the reason for the feature
def test_same_class_rows_differ_only_with_a_context_key(small):
    """Eight samples of one class.  A keyed row is a function of its first ngram (unkeyed) tokens, so two rows are equal exactly when
    those prefixes collide.  "All rows differ" is therefore asserted on a model whose first positions have entropy: the same small
    RAR at logit_scale 1.0, where the oracle's distributions under guidance 4.0 give a 2-token prefix collision probability of
    about 2.6e-5 per pair, 7e-4 for any of the 28 pairs (at the module model's logit_scale 6.0 it is about 0.18: position 0 alone
    collides with probability 0.33, and one such pair was seen on the GPU).  On the sharp model the exact property is asserted."""
    from wmar_amd.models.rar_wrapper import RarARMMWrapper
    from wmar_amd.watermarking.gumbel_watermark import GumbelWatermark
    flat = RarARMMWrapper(None, rar_cfg=SMALL, vq_cfg=SMALL_VQ, rar_state=synth.synth_rar_state(SMALL, seed=1, logit_scale=1.0),
                          vq_state=synth.synth_maskgit_state(SMALL_VQ, seed=1), max_batch=4)
    cond = torch.tensor([7] * 8)
    for m in (flat, small[0]):
        m.use_graph = True
        m.set_watermarker(GumbelWatermark(256, seed=1234, device="cuda"))
        fixed = m.sample(cond, None, apply_watermark=True)
        assert all(torch.equal(fixed[0], fixed[i]) for i in range(8))          # ngram = 0: the image is a function of the class
        m.set_watermarker(GumbelWatermark(256, seed=1234, device="cuda", ngram=2))
        torch.manual_seed(5)
        a = m.sample(cond, None, apply_watermark=True)
        for i in range(8):
            for j in range(i):
                assert torch.equal(a[i], a[j]) == torch.equal(a[i, :2], a[j, :2]), (i, j)
        if m is flat:
            assert all(not torch.equal(a[i], a[j]) for i in range(8) for j in range(i))
        torch.manual_seed(5)
        assert torch.equal(a, m.sample(cond, None, apply_watermark=True))
        torch.manual_seed(6)
        assert not torch.equal(a, m.sample(cond, None, apply_watermark=True))


# ------------------------------------------------------------------ (e) detector
def _np_scores(codes, seed, n, V):
    """numpy restatement: (scores f32 [B, L], mask, n_scored) with W.gumbel_key as the key source."""
    h0 = _h0(seed)
    B, L = codes.shape
    s = np.zeros((B, L), np.float32)
    mask = np.zeros((B, L), np.int8)
    keys = {}
    for b in range(B):
        seen = set()
        for l in range(n, L):
            tup = tuple(int(x) for x in codes[b, l - n:l + 1])
            if tup in seen:
                continue
            seen.add(tup)
            h = h0
            for x in tup[:-1]:
                h ^= x
            if h not in keys:
                keys[h] = W.gumbel_key(h, V)
            mask[b, l] = 1
            s[b, l] = np.float32(-np.log(np.float64(np.float32(1.0) - keys[h][tup[-1]])))
    return s, mask, mask.sum(1).astype(np.int32)


@pytest.mark.parametrize("n,V", [(1, 1024), (2, 256), (4, 16384), (16, 64)])
def test_detector_scores_mask_and_counts_vs_numpy(n, V):
    from wmar_amd.watermarking.gumbel_watermark import GumbelWatermark
    rs = np.random.RandomState(n)
    B, L = 6, 96
    codes = rs.randint(0, V, size=(B, L)).astype(np.int64)
    codes[0] = 5                                                   # one repeated id: a single scored tuple
    codes[1, 40:40 + 2 * (n + 1)] = np.tile(codes[1, 40:41 + n], 2)    # a planted repeat of one (n+1)-tuple
    codes[2, :48] = codes[2, 48:]                                  # the second half repeats the first
    codes[3, -1] = V - 1
    wm = GumbelWatermark(V, seed=42, device="cuda", ngram=n)
    s, mask, ns = (t.cpu().numpy() for t in wm.score_counts(torch.from_numpy(codes)))
    rs_, rm, rn = _np_scores(codes, 42, n, V)
    assert int(ns[0]) == 1
    assert np.array_equal(mask, rm) and np.array_equal(ns, rn)
    assert _same_bits(s, rs_)
    pv, ns2 = wm.detect_counts(torch.from_numpy(codes))
    # p = gammaincc(n_scored, sum) by the same torch function on the same device, fed the numpy restatement's scores: what is left
    # is the order of a 96-term fp64 sum (relative 1e-14) times the function's sensitivity to its argument (below 1e2).  (The CPU and
    # GPU implementations of torch.special.gammaincc themselves differ by 1.1e-9 relative on these inputs.)
    want = torch.special.gammaincc(torch.from_numpy(rn).cuda().double(), torch.from_numpy(rs_.astype(np.float64).sum(1)).cuda())
    np.testing.assert_allclose(pv.cpu().numpy(), want.cpu().numpy(), rtol=1e-11)
    assert torch.equal(wm.detect(torch.from_numpy(codes)), pv) and np.array_equal(ns2.cpu().numpy(), rn)
    with pytest.raises(ValueError):
        wm.detect(torch.zeros(2, n, dtype=torch.int64))
    bad = codes.copy()
    bad[4, 17] = V
    with pytest.raises(RuntimeError):
        wm.scores(torch.from_numpy(bad))
    assert str(wm) == f"gumbel_seed=42_T=1.0_topp=0.0_topk=0_ngram={n}"
    assert str(GumbelWatermark(V, seed=42, device="cuda")) == "gumbel_seed=42_T=1.0_topp=0.0_topk=0"


def test_detector_separates_keyed_codes(small):
    from wmar_amd.watermarking.gumbel_watermark import GumbelWatermark
    m, _ = small
    cond = torch.tensor([3, 500, 77, 9, 12, 999])
    for n in (1, 2, 4):
        wm = GumbelWatermark(256, seed=1234, device="cuda", ngram=n)
        codes, _ = _keyed(m, cond, wm, 11)
        other, _ = _keyed(m, cond, GumbelWatermark(256, seed=4321, device="cuda", ngram=n), 11)
        torch.manual_seed(0)
        plain = m.sample(cond, None, apply_watermark=False)
        p_wm, p_plain, p_other = wm.detect(codes), wm.detect(plain), wm.detect(other)
        print(n, "p keyed", p_wm.tolist(), "plain", p_plain.tolist(), "other key", p_other.tolist())
        assert float(p_wm.max()) < 1e-6 and float(p_plain.min()) > 1e-4 and float(p_other.min()) > 1e-4


def test_detector_null_calibration_2000_uniform_rows():
    """Uniform random codes, V = 1024, L = 256, ngram = 1: the share with p < 0.05 lies in [0.03, 0.07] (binomial 3 sigma around
    0.05 is 0.035-0.065)."""
    from wmar_amd.watermarking.gumbel_watermark import GumbelWatermark
    codes = np.random.RandomState(0).randint(0, 1024, (2000, 256)).astype(np.int64)
    p = GumbelWatermark(1024, seed=42, device="cuda", ngram=1).detect(torch.from_numpy(codes))
    share = float((p < 0.05).double().mean())
    print("share of p < 0.05:", share)
    assert 0.03 <= share <= 0.07


# ------------------------------------------------------------------ (f) determinism
def test_keyed_generation_is_bit_reproducible(small):
    from wmar_amd.watermarking.gumbel_watermark import GumbelWatermark
    m, _ = small
    cond = torch.tensor([3, 500, 77, 9])
    wm = GumbelWatermark(256, seed=1234, device="cuda", ngram=2)
    first, u = _keyed(m, cond, wm, 3, graph=True)
    first = first.clone()
    for rep in range(5):
        assert torch.equal(first, m.sample(cond, None, apply_watermark=True, q=u)), f"graph replay {rep + 1}"
    m.use_graph = False
    assert torch.equal(first, m.sample(cond, None, apply_watermark=True, q=u))
    m.use_graph = True

