"""CPU checks of the hooked generation mode's surroundings: the composed oracle loops against the reference's recorded tokens, the C ABI
of the callback, the `--wm_method custom` flags and detect.py's fallback to a reference-style `detect`."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import hook_processors as HP
from tests.conftest import REPO
from wmar_amd.utils import synth

NEW = ("wmar_cfg_mix", "wmar_gpt_generate_hooked", "wmar_rar_generate_hooked", "wmar_cham_generate_image_hooked")
SMALL = synth.GPTConfig(vocab_size=16384, block_size=16, n_layer=2, n_head=4, n_embd=128)
RCFG = synth.RARConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                       image_seq_len=16, codebook_size=1024, condition_num_classes=1000)


@pytest.fixture(scope="module")
def hv():
    return np.load(os.path.join(REPO, "tests", "golden", "hook_vectors.npz"))


# ------------------------------------------------------------------------------------------------- oracle vs fixture
@pytest.mark.parametrize("proc", list(HP.PROCESSORS))
@pytest.mark.parametrize("tag", list(HP.TAMING_SETTINGS))
def test_taming_oracle_loop_reproduces_reference_tokens(hv, tag, proc):
    tk, tp, T = HP.TAMING_SETTINGS[tag]
    sd = synth.synth_gpt_state(SMALL, seed=3, logit_scale=40.0)
    torch.manual_seed(int(hv["taming_noise_seed"]))
    toks = HP.taming_loop(sd, SMALL.n_head, torch.tensor(HP.TAMING_COND), 16, HP.PROCESSORS[proc](), T, tk, tp)
    assert np.array_equal(toks, hv[f"taming_{tag}_{proc}"])


@pytest.mark.parametrize("proc", list(HP.PROCESSORS))
def test_rar_oracle_loop_reproduces_reference_tokens(hv, proc):
    sd = synth.synth_rar_state(RCFG, seed=2, logit_scale=30.0)
    torch.manual_seed(int(hv["rar_noise_seed"]))
    toks = HP.rar_loop(sd, RCFG, torch.tensor(HP.RAR_CLASSES), HP.PROCESSORS[proc]())
    assert np.array_equal(toks, hv[f"rar_{proc}"])


def test_fixture_processors_change_the_tokens(hv, golden):
    """the recorded runs are not the unprocessed ones: a hook that is never called cannot reproduce them"""
    assert not np.array_equal(hv["taming_k250p92_hash"], golden["loop_nowm_tokens"])
    assert not np.array_equal(hv["taming_k250p92_ban"], golden["loop_nowm_tokens"])
    assert np.array_equal(hv["taming_k250p92_hash"], hv["taming_k250p92_oop_hash"])
    for b in range(4):       # (c): no repeats, and never the class token
        row = hv["taming_plain_ban"][b].tolist()
        assert len(set(row)) == 16 and HP.TAMING_COND[b][0] not in row
        assert len(set(hv["rar_ban"][b].tolist())) == 16


def test_greenlist_processor_is_the_oracle_bias(kat, key_factory):
    """(a) on the CPU == wm_oracle.process_logits (LINEAR h = 1; rows with too short a context untouched)"""
    from oracle import wm_oracle as W
    from wmar_amd.watermarking.gentime_watermark import GentimeWatermark, SeedStrategy, SplitStrategy
    from tests.conftest import load_ids
    cfg = kat["keys"]["rar"]
    alive = load_ids(cfg["alive"])
    dead = sorted(set(range(cfg["vocab"])) - set(alive))
    wm = GentimeWatermark({"alive_ids": torch.tensor(alive), "dead_ids": torch.tensor(dead), "embedding": None}, cfg["vocab"],
                          SeedStrategy(cfg["seed"]), SplitStrategy(cfg["split"]), cfg["h"], 2.0, cfg["gamma"], device="cpu")
    proc = HP.greenlist_from_table(wm)
    rs = np.random.RandomState(0)
    lg = rs.randn(3, cfg["vocab"]).astype(np.float32)
    past = rs.randint(0, cfg["vocab"], size=(3, 4)).astype(np.int64)
    key = key_factory(cfg)
    got = proc(torch.from_numpy(past), torch.from_numpy(lg.copy())).numpy()
    assert np.array_equal(got.view(np.int32), W.process_logits(key, past, lg.copy(), 2.0).view(np.int32))
    assert np.array_equal(proc(torch.from_numpy(past[:, :0]), torch.from_numpy(lg.copy())).numpy(), lg)


# --------------------------------------------------------------------------------------------------------------- ABI
def test_new_symbols_are_declared_listed_and_exported():
    from wmar_amd import _lib
    header = open(os.path.join(REPO, "include", "wmar_hip.h")).read()
    declared = set(re.findall(r"\b(wmar_[a-z0-9_]+)\s*\(", header))
    L = _lib.load()
    for s in NEW:
        assert s in declared and s in _lib.SYMBOLS and hasattr(L, s), s
    assert re.search(r"#define\s+WMAR_ECALLBACK\s+\(-6\)", header) and _lib.WMAR_ECALLBACK == -6


def test_callback_type_matches_the_header(tmp_path):
    """a C function of the documented signature is assignable to wmar_logits_hook (-Werror: an incompatible pointer type fails), and the
    CFUNCTYPE has that argument list"""
    from wmar_amd import _lib
    src = tmp_path / "hook.c"
    src.write_text('#include "wmar_hip.h"\n'
                   'static int my_hook(void* user, int32_t step, int64_t t) { (void)user; return step < 0 || t < 0; }\n'
                   'int main(void) { wmar_logits_hook h = my_hook; return h((void*)0, 0, 0) + (WMAR_ECALLBACK != -6); }\n')
    exe = tmp_path / "hook"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
    assert _lib.LOGITS_HOOK._restype_ is C.c_int
    assert list(_lib.LOGITS_HOOK._argtypes_) == [C.c_void_p, C.c_int32, C.c_int64]
    _lib.load()
    for fn in ("wmar_gpt_generate_hooked", "wmar_rar_generate_hooked", "wmar_cham_generate_image_hooked"):
        at = getattr(_lib.load(), fn).argtypes
        assert at[-3] is _lib.LOGITS_HOOK and at[-2] is C.c_void_p and at[-1] is C.c_void_p, fn


def test_callback_wrapper_keeps_the_exception():
    """ctypes swallows what a callback raises: the wrapper returns non-zero, keeps the exception and finish() re-raises it unchanged"""
    from wmar_amd.models.engine import _LogitsHook

    class Boom(Exception):
        pass

    err = Boom("step 3")

    def proc(past_ids, logits):
        raise err

    h = _LogitsHook(proc, 2, 8, 4, "cpu", positional=False)
    assert h.cfunc(None, 3, 2) == 1
    with pytest.raises(Boom) as e:
        h.finish(-6)
    assert e.value is err
    # shapes, dtypes and the copy-in of a new tensor
    seen = {}

    def proc2(past_ids, logits):
        seen["past"] = (tuple(past_ids.shape), past_ids.stride(), past_ids.dtype)
        seen["logits"] = (tuple(logits.shape), logits.is_contiguous(), logits.dtype)
        return (logits.double() + 1.0)

    h = _LogitsHook(proc2, 2, 8, 4, "cpu", positional=True)
    h.logits.zero_()
    assert h.cfunc(None, 0, 3) == 0 and h.error is None
    assert seen == {"past": ((2, 3), (4, 1), torch.int64), "logits": ((2, 8), True, torch.float32)}
    assert torch.equal(h.logits, torch.ones(2, 8))
    for bad, exc in ((lambda p, l: l[:, :4], ValueError), (lambda p, l: None, TypeError)):
        h = _LogitsHook(bad, 2, 8, 4, "cpu", positional=True)
        assert h.cfunc(None, 0, 1) == 1
        with pytest.raises(exc):
            h.finish(-6)


# --------------------------------------------------------------------------------------------------------------- CLI
def _gen_args(*argv):
    import generate
    return generate.get_parser().parse_args(list(argv))


def test_custom_method_parses_and_needs_its_factory(monkeypatch, capsys):
    import detect
    import generate
    a = _gen_args("--model", "taming", "--wm_method", "custom", "--wm_factory", "tests.test_hook_reference:factory")
    assert a.wm_method == "custom" and a.wm_factory == "tests.test_hook_reference:factory"
    generate.check_wm_args(a)
    with pytest.raises(ValueError, match="needs --wm_factory"):
        generate.check_wm_args(_gen_args("--model", "taming", "--wm_method", "custom"))
    with pytest.raises(ValueError, match="only read with --wm_method custom"):
        generate.check_wm_args(_gen_args("--model", "taming", "--wm_method", "gentime", "--wm_factory", "a.b:c"))
    with pytest.raises(ValueError, match="pkg.module:callable"):
        generate.check_wm_args(_gen_args("--model", "taming", "--wm_method", "custom", "--wm_factory", "nocolon"))
    for main, argv in ((generate.main, ["generate.py", "--outdir", "x"]), (detect.main, ["detect.py", "--images", "x", "--out", "y"])):
        monkeypatch.setattr("sys.argv", argv + ["--model", "taming", "--wm_method", "custom"])
        with pytest.raises(SystemExit) as e:          # stops at the parser, before any model is built
            main()
        assert e.value.code == 2 and "needs --wm_factory" in capsys.readouterr().err


class ForeignWatermark:
    """What a watermark research code base offers: the reference's interface and nothing else."""

    def __init__(self, model, args):
        self.model, self.args = model, args

    def spawn_logit_processor(self):
        return HP.hash_bias

    def detect(self, codes):
        return torch.full((codes.shape[0],), 0.25, dtype=torch.float64)

    def __str__(self):
        return "foreign-hash"


def factory(model, args):
    return ForeignWatermark(model, args)


def test_build_watermarker_calls_the_factory():
    from wmar_amd import cli
    a = _gen_args("--model", "taming", "--wm_method", "custom", "--wm_factory", "tests.test_hook_reference:factory")

    class Model:
        device = "cpu"

        def get_total_vocab_size(self):
            return 16

    m = Model()
    wm = cli.build_watermarker(a, m)
    assert type(wm).__name__ == "ForeignWatermark" and wm.model is m and wm.args is a and str(wm) == "foreign-hash"


def test_detect_scores_through_detect_without_counts(monkeypatch, tmp_path):
    import detect
    from PIL import Image
    from wmar_amd import cli

    class Model:
        device = "cpu"

        def get_total_vocab_size(self):
            return 16

        def codes_from_pil(self, images):
            return torch.zeros(len(images), 4, dtype=torch.int64)

    monkeypatch.setattr(cli, "build_model", lambda args, device, seed: Model())
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    Image.new("RGB", (5, 7)).save(tmp_path / "a.png")
    out = tmp_path / "o.json"
    monkeypatch.setattr("sys.argv", ["detect.py", "--model", "taming", "--wm_method", "custom", "--wm_factory",
                                     "tests.test_hook_reference:factory", "--images", str(tmp_path), "--out", str(out)])
    assert detect.main() == 0
    recs = json.load(open(out))
    assert len(recs) == 1 and recs[0]["pvalue"] == 0.25 and "n_scored" not in recs[0] and "n_green" not in recs[0]
