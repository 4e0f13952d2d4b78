"""CPU checks of the detection entry point's surface: flags, the checks it shares with generate.py, file listing, C ABI declarations."""
import os
import re

import pytest

from tests.conftest import REPO

NEW = ("wmar_resample_coeffs", "wmar_image_ingest")


def _args(*argv):
    import detect
    return detect.get_parser().parse_args(list(argv))


def test_parser_takes_generate_flags_and_its_own():
    import detect
    import generate
    a = _args("--model", "taming", "--wm_method", "gentime", "--wm_seed_strategy", "linear", "--wm_split_strategy", "stratifiedrand",
              "--wm_context_size", "1", "--wm_delta", "2.0", "--wm_gamma", "0.25", "--images", "a.png", "b.png", "--batch_size", "7",
              "--out", "r.json", "--synthetic", "1", "--synthetic_config", "harness")
    assert a.images == ["a.png", "b.png"] and a.batch_size == 7 and a.out == "r.json" and a.synthetic is True
    generate.check_wm_args(a)
    assert _args("--images", "dir").images == ["dir"]
    g = {x.dest for x in generate.get_parser()._actions}
    d = {x.dest for x in detect.get_parser()._actions}
    assert g < d and d - g == {"images", "out"}
    generate.check_wm_args(_args("--model", "rar", "--wm_method", "gumbel", "--wm_context_size", "2", "--images", "x"))


@pytest.mark.parametrize("model", ["taming", "chameleon7b"])
def test_gumbel_stays_rar_only(model, monkeypatch, capsys):
    import detect
    import generate
    with pytest.raises(ValueError, match="no Gumbel-key generation"):
        generate.check_wm_args(_args("--model", model, "--wm_method", "gumbel", "--images", "x", "--out", "y"))
    monkeypatch.setattr("sys.argv", ["detect.py", "--images", "x", "--out", "y", "--model", model, "--wm_method", "gumbel"])
    with pytest.raises(SystemExit) as e:          # stops at the parser, before any model is built
        detect.main()
    assert e.value.code == 2 and "no Gumbel-key generation" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--out", "y", "--model", "taming", "--wm_method", "gentime"],
                                  ["--images", "x", "--model", "taming", "--wm_method", "gentime"],
                                  ["--images", "x", "--out", "y", "--model", "taming", "--wm_method", "none"]])
def test_missing_flags_stop_at_the_parser(argv, monkeypatch):
    import detect
    monkeypatch.setattr("sys.argv", ["detect.py"] + argv)
    with pytest.raises(SystemExit) as e:
        detect.main()
    assert e.value.code == 2


def test_list_images_sorts(tmp_path):
    import detect
    for n in ("b.png", "a.jpg", "c.png"):
        (tmp_path / n).write_bytes(b"x")
    (tmp_path / "sub").mkdir()
    assert [os.path.basename(f) for f in detect.list_images([str(tmp_path)])] == ["a.jpg", "b.png", "c.png"]
    assert detect.list_images(["z.png", "y.png"]) == ["y.png", "z.png"]


def test_detect_builds_model_and_watermarker_through_the_shared_helper(monkeypatch, tmp_path):
    """detect.main hands the parsed flags to cli.build_model / cli.build_watermarker (what generate.py calls too) and scores what
    the model's codes_from_pil returns"""
    import torch
    import detect
    from PIL import Image
    from wmar_amd import cli
    seen = {}

    class Model:
        def codes_from_pil(self, images):
            seen["n"] = len(images)
            return torch.zeros(len(images), 4, dtype=torch.int64)

    class Wm:
        def detect_counts(self, codes):
            return torch.full((codes.shape[0],), 0.5, dtype=torch.float64), torch.full((codes.shape[0],), 3, dtype=torch.int32)

    def build_model(args, device, seed):
        seen["model"] = (args.model, device, seed)
        return Model()

    def build_watermarker(args, model):
        seen["wm"] = (args.wm_method, isinstance(model, Model))
        return Wm()

    monkeypatch.setattr(cli, "build_model", build_model)
    monkeypatch.setattr(cli, "build_watermarker", build_watermarker)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    Image.new("RGB", (5, 7)).save(tmp_path / "a.png")
    (tmp_path / "b.png").write_bytes(b"junk")
    out = tmp_path / "o.json"
    monkeypatch.setattr("sys.argv", ["detect.py", "--model", "rar", "--wm_method", "gumbel", "--seed", "5", "--images", str(tmp_path),
                                     "--out", str(out)])
    assert detect.main() == 1
    assert seen == {"model": ("rar", "cuda:0", 5), "wm": ("gumbel", True), "n": 1}
    import json
    recs = json.load(open(out))
    assert [os.path.basename(r["file"]) for r in recs] == ["a.png", "b.png"]
    assert recs[0]["pvalue"] == 0.5 and recs[0]["n_scored"] == 3 and (recs[0]["width"], recs[0]["height"]) == (5, 7)
    assert "error" in recs[1] and "pvalue" not in recs[1]


def test_new_symbols_are_declared_and_exported():
    from wmar_amd import _lib
    header = open(os.path.join(REPO, "include", "wmar_hip.h")).read()
    declared = set(re.findall(r"\b(wmar_[a-z0-9_]+)\s*\(", header))
    L = _lib.load()
    for s in NEW:
        assert s in declared and s in _lib.SYMBOLS and hasattr(L, s), s


def test_image_desc_matches_the_compiled_header(tmp_path):
    import ctypes as C
    import subprocess
    from wmar_amd import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wmar_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(wmar_image_desc));']
    for fname, _ in _lib.ImageDesc._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(wmar_image_desc, {fname}));')
    lines += ['return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(_lib.ImageDesc)
    for fname, _ in _lib.ImageDesc._fields_:
        assert int(got[fname]) == getattr(_lib.ImageDesc, fname).offset, fname
