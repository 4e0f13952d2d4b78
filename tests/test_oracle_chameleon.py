"""Chameleon host pieces against the reference's own outputs (tests/golden/chameleon_vectors.npz, made by importing
deps/chameleon/inference/{logits_processor,token_selector,vocab}.py and the HF warpers).  CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import cham_oracle as CO
from oracle import wm_oracle as W
from tests.conftest import REPO
from tests.golden.make_golden import synth_vocab_map


@pytest.fixture(scope="module")
def cv():
    return np.load(os.path.join(REPO, "tests", "golden", "chameleon_vectors.npz"))


def test_vocab_mirrors(cv):
    from wmar_amd.models.chameleon import VocabInfo, VocabTranslation
    vi = VocabInfo(synth_vocab_map())
    assert vi.image_tokens == cv["cham_image_tokens"].tolist()
    assert vi.text_tokens == cv["cham_text_tokens"].tolist()
    assert vi.special_tokens == cv["cham_special_tokens"].tolist()
    assert [vi.bos_id, vi.eos_id, vi.boi_id, vi.eoi_id, vi.pad_id, vi.eot_id] == cv["cham_ids"].tolist()
    assert (vi.begin_image, vi.end_image, vi.begin_sequence) == (vi.boi_id, vi.eoi_id, vi.bos_id)
    vt = VocabTranslation(vi)
    assert np.array_equal(vt.convert_bpe2img(torch.from_numpy(cv["cham_bpe_batch"])).numpy(), cv["cham_bpe2img"])
    assert np.array_equal(vt.convert_img2bp2(torch.from_numpy(cv["cham_img_batch"])).numpy(), cv["cham_img2bpe"])


@pytest.mark.parametrize("name,seed", [("fixed", "fixed"), ("linear", "linear"), ("nowm", None)])
def test_sampling_chain_equals_reference(cv, name, seed):
    h, delta, temp, top_p = cv[f"cham_{name}_params"]
    alive = cv["cham_image_tokens"]
    V = cv["cham_logits3"].shape[1]
    dead = np.array(sorted(set(range(V)) - set(alive.tolist())), dtype=np.int64)
    key = W.KeyParams(alive, dead, V, 0.25, seed=seed) if seed else None
    tok, lg = CO.sample_step(torch.from_numpy(cv["cham_logits3"]), cv[f"cham_{name}_q"], float(temp), float(top_p), 3.0, 1.2,
                             allow_ids=alive, key=key, past_ids=cv["cham_input_ids"], delta=float(delta))
    ref = cv[f"cham_{name}_processed"] * float(temp)       # the fixture holds logits after temperature and top-p
    kept = np.isfinite(ref)
    np.testing.assert_allclose(lg[kept], ref[kept], rtol=2e-6, atol=2e-6)
    assert np.array_equal(tok, cv[f"cham_{name}_tok"])


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("hd,kv,qk", [(64, None, True), (64, 1, False), (128, 1, True), (128, None, False)])
def test_prefix_equals_incremental(hd, kv, qk, fold):
    """`prefix` (one causally masked pass per layer) against `forward_tokens` fed position by position: 72 positions (the engine's
    attention reads 16- / 32-row chunks; several of each), MHA and GQA, qk-norm on and off, both rounding modes.  The two forms round
    the same values to bf16 at the same points but sum in different orders (matrix blocking), so a bf16 flip may propagate: measured
    max |d| is one bf16 ulp of the largest logits (0.0625 .. 0.125 at logit std 4, 1.5 .. 3.1 % of std) and the mean 0.07 .. 0.24 % of
    std; asserted here with the ulp term of the engine gate (tests/test_gpu_chameleon.py::_close) and a third / half of its std terms."""
    from wmar_amd.utils import synth
    cfg = synth.ChameleonConfig(dim=256, n_layers=2, n_heads=256 // hd, n_kv_heads=kv or 256 // hd, vocab_size=1024, multiple_of=64,
                                qk_normalization=qk)
    sd = synth.synth_chameleon_state(cfg, seed=11, logit_scale=4.0)
    R, Tn = 3, 72
    rs = np.random.RandomState(hd + (kv or 0) + 2 * qk)
    seq = torch.from_numpy(rs.randint(0, cfg.vocab_size, size=(R, Tn)).astype(np.int64))
    got = CO.prefix(sd, cfg, seq, None, fold)
    assert got.shape == (R, Tn, cfg.vocab_size)
    cache = CO.Cache(cfg.n_layers, R)
    ref = torch.stack([CO.forward_tokens(sd, cfg, seq[:, t], torch.full((R,), t), cache, fold) for t in range(Tn)], 1)
    d = (got - ref).abs()
    scale, top = float(ref.std()), float(ref.abs().max())
    sub = CO.prefix(sd, cfg, seq, [0, 33, Tn - 1], fold)         # the head at selected positions only (other blocking: an ulp apart)
    assert float((sub - got[:, [0, 33, Tn - 1]]).abs().max()) <= 2.0 ** -7 * top
    # arg-max: equal on every (row, position) unless the two candidates are within one bf16 ulp of each other in the reference (ties)
    am_g, am_r = got.argmax(-1), ref.argmax(-1)
    gap = (ref.gather(-1, am_r[..., None]) - ref.gather(-1, am_g[..., None])).squeeze(-1)
    print(f"prefix vs incremental hd {hd} kv {kv} qk {qk} fold {fold}: max |d| {float(d.max()):.4f} = {float(d.max()) / scale:.4f} std, "
          f"mean {float(d.mean()) / scale:.5f} std, arg-max differs at {int((am_g != am_r).sum())} of {R * Tn} (max gap {float(gap.max()):.4f})")
    assert float(d.max()) <= 0.01 * scale + 2.0 ** -7 * top
    assert float(d.mean()) <= 0.004 * scale
    assert float(gap.max()) <= 2.0 ** -7 * top
