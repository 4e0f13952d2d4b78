"""Generate tests/golden/hook_vectors.npz: the tokens the REFERENCE's generation loops return under foreign logit processors.

Usage (build machine; the GPU box never runs this):
    python tests/golden/make_hook_vectors.py --ref /path/to/wmar

The reference is imported from its checkout (never copied), with the stand-in modules of make_golden._stubs for the packages it
imports that are absent here.  Everything written is data: token ids and the noise seeds.

Loops and models are those of the existing fixtures:
  Taming  sample_with_past (mingpt.py:326-368) on tests/test_gpu_gpt.py's SMALL (synth_gpt_state(seed=3, logit_scale=40)), the
          class tokens of golden["loop_cond"], 16 steps, sampling settings "k250p92" and "plain";
  RAR     RAR.generate (rar.py:408-459) on the reduced RAR of rar_vectors (seed 2, logit scale 30, classes 3 / 977 / 0 / 512,
          guidance 4.0).
Processors (tests/hook_processors.py): "hash" (b), "ban" (c), "oop_hash" (d)o(b).  Keys: `taming_<setting>_<proc>`, `rar_<proc>`
int64 [4, 16]; `taming_noise_seed`, `rar_noise_seed` (torch.manual_seed in front of the loop).

The GPU tests demand exact token equality, so no recorded decision may sit on a knife edge: for every case the composed oracle loop
(tests/hook_processors.py) is re-run 8 times with every step's logits perturbed by seeded uniform noise of +-5e-4 -- the logit
tolerance tests/test_gpu_gpt.py grants the engine -- and all 8 runs must return the reference's tokens.  If a noise seed fails for any
case of its model (starting from the existing 11 / 21), the next one is taken; the seed used is stored in the file.
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

N_JITTER = 8


class AD(dict):
    def __getattr__(self, k):
        v = self[k]
        return AD(v) if isinstance(v, dict) else v

    def get(self, k, d=None):
        return dict.get(self, k, d)


def taming_cases(seed):
    """{key: tokens} of the reference under every processor and setting with noise seed `seed`, or None if a case is not robust."""
    import torch
    from deps.taming.modules.transformer.mingpt import GPT, sample_with_past
    from tests import hook_processors as HP
    from wmar_amd.utils import synth

    cfg = synth.GPTConfig(vocab_size=16384, block_size=16, n_layer=2, n_head=4, n_embd=128)
    sd = synth.synth_gpt_state(cfg, seed=3, logit_scale=40.0, with_mask=True)
    gpt = GPT(vocab_size=cfg.vocab_size, block_size=cfg.block_size, n_layer=cfg.n_layer, n_head=cfg.n_head, n_embd=cfg.n_embd)
    gpt.load_state_dict(sd, strict=True)
    gpt.eval()
    osd = {k: v for k, v in sd.items() if not k.endswith("attn.mask")}
    cond = torch.tensor(HP.TAMING_COND, dtype=torch.long)
    out = {}
    for tag, (tk, tp, T) in HP.TAMING_SETTINGS.items():
        for name, make in HP.PROCESSORS.items():
            torch.manual_seed(seed)
            with contextlib.redirect_stdout(io.StringIO()):
                toks = sample_with_past(cond, gpt, steps=16, temperature=T, sample_logits=True, top_k=tk, top_p=tp,
                                        logit_processor=make()).numpy()
            torch.manual_seed(seed)
            base = HP.taming_loop(osd, cfg.n_head, cond, 16, make(), T, tk, tp)
            if not np.array_equal(base, toks):
                print(f"  taming {tag} {name} seed {seed}: the composed oracle loop differs from the reference")
                return None
            for j in range(N_JITTER):
                torch.manual_seed(seed)
                if not np.array_equal(HP.taming_loop(osd, cfg.n_head, cond, 16, make(), T, tk, tp, jitter=HP.uniform_jitter(1000 + j)), toks):
                    print(f"  taming {tag} {name} seed {seed}: jitter run {j} changes a token")
                    return None
            out[f"taming_{tag}_{name}"] = toks
    return out


def rar_cases(seed):
    import torch
    from deps.rar.modeling.rar import RAR
    from tests import hook_processors as HP
    from wmar_amd.utils import synth

    rcfg = synth.RARConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                           image_seq_len=16, codebook_size=1024, condition_num_classes=1000)
    cfg = AD(model=dict(vq_model=dict(codebook_size=1024),
                        generator=dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                                       image_seq_len=16, condition_num_classes=1000, dropout=0.0, attn_drop=0.0)))
    sd = synth.synth_rar_state(rcfg, seed=2, logit_scale=30.0)
    gen = RAR(cfg).eval()
    gen.load_state_dict(sd, strict=True)
    gen.set_random_ratio(0)
    cond = torch.tensor(HP.RAR_CLASSES, dtype=torch.long).view(-1, 1)
    out = {}
    for name, make in HP.PROCESSORS.items():
        torch.manual_seed(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            toks = gen.generate(condition=cond, guidance_scale=4.0, guidance_scale_pow=0.0, randomize_temperature=1.0,
                                logit_processor=make()).numpy()
        torch.manual_seed(seed)
        base = HP.rar_loop(sd, rcfg, cond.view(-1), make())
        if not np.array_equal(base, toks):
            print(f"  rar {name} seed {seed}: the composed oracle loop differs from the reference")
            return None
        for j in range(N_JITTER):
            torch.manual_seed(seed)
            if not np.array_equal(HP.rar_loop(sd, rcfg, cond.view(-1), make(), jitter=HP.uniform_jitter(2000 + j)), toks):
                print(f"  rar {name} seed {seed}: jitter run {j} changes a token")
                return None
        out[f"rar_{name}"] = toks
    return out


def first_robust(cases, seed0, what):
    for seed in range(seed0, seed0 + 32):
        got = cases(seed)
        if got is not None:
            print(f"{what}: noise seed {seed}")
            return seed, got
    raise SystemExit(f"{what}: no robust noise seed in {seed0}..{seed0 + 31}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (facebookresearch/wmar)")
    args = ap.parse_args()
    from make_golden import _stubs
    tmp = tempfile.mkdtemp(prefix="wmar_stubs_")
    _stubs(tmp)
    sys.path[:0] = [tmp, args.ref, REPO]
    out = {}
    seed, got = first_robust(taming_cases, 11, "taming")
    out.update(got)
    out["taming_noise_seed"] = np.array(seed, dtype=np.int64)
    seed, got = first_robust(rar_cases, 21, "rar")
    out.update(got)
    out["rar_noise_seed"] = np.array(seed, dtype=np.int64)
    path = os.path.join(HERE, "hook_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
