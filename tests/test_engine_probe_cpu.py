"""The device-free parts of tests/engine_probe.py: the plan parser on one plan text per engine (as wmar_*_probe_plan formats them),
the creation-time environment switches, and the element types each engine's test file declares for its buffers."""
import os

import pytest
import torch

from tests.engine_probe import engine_env, parse_plan

GPT_KERNELS = ("qkv=k_qkvx_bx<6> (bf16 pipe, 7 K slices);attn=k_attn_decode<64,2>;proj=k_bx_xr<6,4> (bf16 pipe, 4 K slices + XCD-local reduction: "
               "residual fold and LN2 statistics inside);resid=k_resid_stats;resid_launches_per_step=1;fc1=k_fc1x (fp32 MFMA, 24-column tiles, whole K);"
               "fc2=k_gemm<EPI_PACKED> (fp32 MFMA, 5/+1 K slices);head=k_gemm<EPI_LOGITS,LN> (fp32 MFMA);barrier_fallbacks=0")
GPT_PLAN = ("small=0 MT=2 S_qx=7 nkeep=4 S_qkv=1 S_proj=4 S_fc2=5 fc2_hi=16 nch=12 nch_ln2=16 pingpong=1 x_head=x attn_waves=2 rowmajor=1 proj=bx_xr "
            "head=1,256 fc1_tiles=0 head_tiles=2 xcd_ok=1 xr_eligible=1 barrier_fallbacks=0 stages=EMBED,QKV,ATTN,PROJ,FC1,FC2,RESID_OUT,HEAD kernels=" + GPT_KERNELS)
RAR_KERNELS = ("embed=k_rar_embed;adaln=k_gemm<2,EPI_PACKED>;mod_in=k_modulate;qkv=k_bx<2,5,4> rowmajor;attn=k_attn_decode80<2> rowmajor;proj=k_bx<1,5,4>;"
               "resid_attn=k_resid_mod<1,1,0>;resid_mlp=k_resid_mod<5,1,0>;fc1=k_gemm<4,EPI_GELU> planes;fc2=k_bx<2,4,4>;head=k_gemm<2,EPI_LOGITS>")
RAR_PLAN = ("MT=4 MTc=2 bx=1 ada_bx=0 fc1_bx=0 rowmajor=1 S_qkv=1 S_proj=1 S_fc2=5 PER_qkv=5 PER_proj=5 PER_fc2=4 nch=4 nrm=4 kpw=1 fused=1 fallbacks=0 "
            "ada_tiles=2 fc1_tiles=4 head_tiles=2 attn_waves=2 stages=EMBED,ADALN,MOD_IN,QKV,HEAD kernels=" + RAR_KERNELS)
CHAM_KERNELS = "k_bgemm<4,SLAB>;k_bgemm<4,LOGITS>;k_cham_attn<128,2>"                # no role=kernel pairs: no `roles`
CHAM_PLAN = "MT=4 sk_qkv=96,48,3 sk_o=32,64,2 sk_13=64,128,4 sk_2=32,64,1 sk_head=256,2,1 kernels=" + CHAM_KERNELS
CHAM_TEXT = {"MT": "4", "sk_qkv": "96,48,3", "sk_o": "32,64,2", "sk_13": "64,128,4", "sk_2": "32,64,1", "sk_head": "256,2,1", "kernels": CHAM_KERNELS}
PLANS = {
    "gpt": (GPT_PLAN, {}, {
        "small": 0, "MT": 2, "S_qx": 7, "nkeep": 4, "S_qkv": 1, "S_proj": 4, "S_fc2": 5, "fc2_hi": 16, "nch": 12, "nch_ln2": 16, "pingpong": 1, "x_head": "x",
        "attn_waves": 2, "rowmajor": 1, "proj": "bx_xr", "head": "1,256", "fc1_tiles": 0, "head_tiles": 2, "xcd_ok": 1, "xr_eligible": 1, "barrier_fallbacks": 0,
        "stages": ["EMBED", "QKV", "ATTN", "PROJ", "FC1", "FC2", "RESID_OUT", "HEAD"], "kernels": GPT_KERNELS,
        "roles": {"qkv": "k_qkvx_bx<6> (bf16 pipe, 7 K slices)", "attn": "k_attn_decode<64,2>",
                  "proj": "k_bx_xr<6,4> (bf16 pipe, 4 K slices + XCD-local reduction: residual fold and LN2 statistics inside)", "resid": "k_resid_stats",
                  "resid_launches_per_step": "1", "fc1": "k_fc1x (fp32 MFMA, 24-column tiles, whole K)", "fc2": "k_gemm<EPI_PACKED> (fp32 MFMA, 5/+1 K slices)",
                  "head": "k_gemm<EPI_LOGITS,LN> (fp32 MFMA)", "barrier_fallbacks": "0"}}),
    "rar": (RAR_PLAN, {}, {
        "MT": 4, "MTc": 2, "bx": 1, "ada_bx": 0, "fc1_bx": 0, "rowmajor": 1, "S_qkv": 1, "S_proj": 1, "S_fc2": 5, "PER_qkv": 5, "PER_proj": 5, "PER_fc2": 4,
        "nch": 4, "nrm": 4, "kpw": 1, "fused": 1, "fallbacks": 0, "ada_tiles": 2, "fc1_tiles": 4, "head_tiles": 2, "attn_waves": 2,
        "stages": ["EMBED", "ADALN", "MOD_IN", "QKV", "HEAD"], "kernels": RAR_KERNELS,
        "roles": {"embed": "k_rar_embed", "adaln": "k_gemm<2,EPI_PACKED>", "mod_in": "k_modulate", "qkv": "k_bx<2,5,4> rowmajor", "attn": "k_attn_decode80<2> rowmajor",
                  "proj": "k_bx<1,5,4>", "resid_attn": "k_resid_mod<1,1,0>", "resid_mlp": "k_resid_mod<5,1,0>", "fc1": "k_gemm<4,EPI_GELU> planes",
                  "fc2": "k_bx<2,4,4>", "head": "k_gemm<2,EPI_LOGITS>"}}),
    "cham": (CHAM_PLAN, dict(list_keys=(), ints=False), CHAM_TEXT),                     # as the Chameleon file reads it: every value text
    "no-kernels": ("small=1 MT=2 head=ntw2 stages=EMBED", {}, {"small": 1, "MT": 2, "head": "ntw2", "stages": ["EMBED"]}),   # neither `kernels` nor `roles`
}


@pytest.mark.parametrize("case", sorted(PLANS))
def test_parse_plan(case):
    text, kwargs, want = PLANS[case]
    assert parse_plan(text, **kwargs) == want


def test_engine_env_restores_values_and_absence(monkeypatch):
    unset, zero = "WMAR_TEST_ENV_UNSET", "WMAR_TEST_ENV_ZERO"
    monkeypatch.delenv(unset, raising=False)
    monkeypatch.setenv(zero, "0")
    with engine_env((unset, zero)):
        assert os.environ[unset] == "1" and os.environ[zero] == "1"
    assert unset not in os.environ and os.environ[zero] == "0"
    with pytest.raises(RuntimeError):
        with engine_env((unset, zero)):
            assert os.environ[unset] == "1" and os.environ[zero] == "1"
            raise RuntimeError("creation failed")
    assert unset not in os.environ and os.environ[zero] == "0"


def test_buffer_dtypes_of_the_three_engines():
    """a buffer missing from DTYPES would silently be float32: the maps are written out a second time here"""
    from tests import test_gpu_cham_kernels, test_gpu_gpt_kernels, test_gpu_rar_kernels
    f64, i64, i32, i16, f32 = torch.float64, torch.int64, torch.int32, torch.int16, torch.float32
    gpt, rar, cham = test_gpu_gpt_kernels.Probe, test_gpu_rar_kernels.Probe, test_gpu_cham_kernels.Probe
    assert (gpt.ENGINE, rar.ENGINE, cham.ENGINE) == ("gpt", "rar", "cham")
    assert gpt.DTYPES == {"stats": f64, "stats_q": f64, "yq": i16} and not gpt.U64
    assert rar.DTYPES == {"stats": f64, "part": i64, "ids": i64, "cond_ids": i64, "ctr": i32, "xq": i16, "yq": i16, "hq": i16, "scq": i16}
    assert set(rar.U64) == {"part"}                                        # int64 on the device, read as uint64
    assert cham.DTYPES == {"x": i16, "y": i16, "hbuf": i16, "slabs": f32, "big_slabs": f32, "ssq": f64, "kcache": i16, "vcache": i16, "rope": f32,
                           "wqkv": i16, "wo": i16, "w13": i16, "w2": i16, "whead": i16} and not cham.U64
