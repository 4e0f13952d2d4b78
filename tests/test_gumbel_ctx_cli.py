"""CPU checks of the context-keyed Gumbel watermark's surface: CLI flags, C ABI declarations and exports, constructor."""
import inspect
import os
import re

import pytest

from tests.conftest import REPO

NEW = ("wmar_gumbel_key_rows", "wmar_rar_generate_gumbel_ctx", "wmar_gumbel_score_ctx")


def _args(*argv):
    import generate
    return generate.get_parser().parse_args(["--outdir", "x", "--conditioning", "1", *argv])


def test_parser_accepts_gumbel_for_rar():
    import generate
    a = _args("--model", "rar", "--wm_method", "gumbel", "--wm_context_size", "2")
    assert a.wm_method == "gumbel" and a.wm_gumbel_seed == 42 and a.wm_context_size == 2
    generate.check_wm_args(a)
    assert _args("--model", "rar", "--wm_method", "gumbel", "--wm_gumbel_seed", "7", "--seed", "3").wm_gumbel_seed == 7
    generate.check_wm_args(_args("--model", "taming", "--wm_method", "gentime"))


@pytest.mark.parametrize("model", ["taming", "chameleon7b"])
def test_gumbel_is_rejected_with_a_reason_for_models_without_the_loop(model, monkeypatch, capsys):
    import generate
    with pytest.raises(ValueError, match="no Gumbel-key generation"):
        generate.check_wm_args(_args("--model", model, "--wm_method", "gumbel"))
    monkeypatch.setattr("sys.argv", ["generate.py", "--outdir", "x", "--conditioning", "1", "--model", model, "--wm_method", "gumbel"])
    with pytest.raises(SystemExit) as e:          # the CLI stops at the parser, before any model is built
        generate.main()
    assert e.value.code == 2 and "no Gumbel-key generation" in capsys.readouterr().err


def test_context_size_outside_the_window_bound_is_rejected():
    import generate
    with pytest.raises(ValueError):
        generate.check_wm_args(_args("--model", "rar", "--wm_method", "gumbel", "--wm_context_size", "17"))


def test_new_symbols_are_declared_and_exported():
    from wmar_amd import _lib
    header = open(os.path.join(REPO, "include", "wmar_hip.h")).read()
    declared = set(re.findall(r"\b(wmar_[a-z0-9_]+)\s*\(", header))
    L = _lib.load()
    for s in NEW:
        assert s in declared and s in _lib.SYMBOLS and hasattr(L, s), s


def test_constructor_takes_ngram_last_and_names_it():
    from wmar_amd.watermarking.gumbel_watermark import GumbelWatermark
    assert list(inspect.signature(GumbelWatermark.__init__).parameters)[1:] == ["vocab_size", "seed", "temperature", "top_p", "top_k",
                                                                                "device", "ngram"]
    w = GumbelWatermark(1024, ngram=1, device="cpu")
    assert w.ngram == 1 and str(w) == "gumbel_seed=42_T=1.0_topp=0.0_topk=0_ngram=1"
    assert str(GumbelWatermark(1024, device="cpu")) == "gumbel_seed=42_T=1.0_topp=0.0_topk=0"
    for n in (-1, 17):
        with pytest.raises(ValueError):
            GumbelWatermark(1024, ngram=n, device="cpu")
    with pytest.raises(ValueError):
        GumbelWatermark(65536, ngram=1, device="cpu")


def test_window_hash_is_h0_xor_the_ids():
    import torch
    from wmar_amd.watermarking.gumbel_watermark import empty_window_hash, get_wm_window_hash
    ng = torch.tensor([[3, 5, 9], [0, 0, 0], [1023, 1, 2]])
    h0 = empty_window_hash(42)
    assert get_wm_window_hash(ng, 42).tolist() == [h0 ^ 3 ^ 5 ^ 9, h0, h0 ^ 1023 ^ 1 ^ 2]
    assert get_wm_window_hash(ng[:, :0], 42).tolist() == [42, 42, 42]
