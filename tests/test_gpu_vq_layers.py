"""MI355X: every VQGAN kernel variant alone against a float64 reference (wmar_amd/csrc/vqgan.hip through the wmar_vq_probe_* entries).

The end-to-end tests (test_gpu_vqgan.py, test_gpu_vq_fullsize.py, test_gpu_rar.py, test_gpu_vq_paths.py) compare whole networks
with the fp32 oracle at atol 2e-4 .. 8e-4 -- 40 to 100 times what a correct build produces, and blind to an error confined to one
tile edge, channel group or dispatch branch.  Here each case names the kernel it means to cover and ASSERTS that the dispatch
(run_conv / run_gn / run_vq_argmin / the attention core, reporting their own decisions) launched it.

Gates (none of them measured on the code under test):
  impulse   one product per output: |y - w x| <= 2^-21 |w x|.  k_conv_bx adds six piece products into an fp32 accumulator (six
            roundings) and drops < 2^-24 (bx_split.h): 7 x 2^-24 at worst; the fp32 kernels round once.  Padding outputs exactly 0;
            bf16-exact operands give the exact product.  tests/test_vq_layer_reference.py shows on the CPU that a kernel which
            loses one second-order piece product puts 3/4 of the outputs above this gate.
  dense     max |y - exact| / (sum|w x| + |bias| + |res|) <= 2 x the same figure of a sequential fp32 multiply-add chain on the
            same data ("fp32 accuracy" = an fp32 contraction in the worst reasonable order; 2 x covers the spread of a maximum
            over 10^4 outputs; k_conv_few is such a chain).
  epilogue  zero weights: bit-equal to fl32(bias + res), padding output channels exactly 0.
  padding   garbage in the input's padding channels changes no bit.
  GroupNorm elementwise error of the staged activation <= 4 x the error of torch's fp32 CPU silu(group_norm(x)) (the loader's
            __expf scales its argument: up to |r| ulp); statistics within the final fp32 roundings of fp64 sums.
  attention <= 4 x torch's fp32 CPU softmax(q k^T scale) v; an all-equal row gives the plain mean of V to 2^-21 of mean|V|.
  argmin    d64(chosen) <= min d64 + 8 x 2^-24 (|z|^2 + |e_chosen|^2) for EVERY pixel; exact duplicates: the lower index wins.

The measured ratios (printed on lines starting with VQLAYER, run with -s) are tabulated in DESIGN.md, "exactness".
(reference: deps/taming/modules/diffusionmodules/model.py:30-193, deps/taming/modules/vqvae/quantize.py:272-285)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import vq_layer_checks as K
from tests.vq_layer_checks import ConvCase as C

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The smallest shapes that reach each instantiation, read from run_conv's dispatch.
CONV_CASES = [
    C("k_conv<1>", 3, 32, 3, 8),
    C("k_conv<1>", 40, 32, 3, 16),                      # a full 32-channel round plus an 8-channel round
    C("k_conv<1>", 32, 32, 3, 16, stride=2),
    C("k_conv<2>", 3, 64, 3, 16),
    C("k_conv<4>", 3, 128, 3, 16),
    C("k_conv<4>", 8, 160, 1, 8),                       # 5 output tiles: a second group with three inactive waves
    C("k_conv_bx<1,1>", 32, 32, 1, 8),
    C("k_conv_bx<1,3>", 32, 32, 3, 8),
    C("k_conv_bx<1,3>", 32, 3, 3, 8),                   # too small for k_conv_few
    C("k_conv_bx<2,1>", 64, 64, 1, 8),
    C("k_conv_bx<2,1>", 64, 64, 1, 24),
    C("k_conv_bx<2,3>", 64, 64, 3, 8),
    C("k_conv_bx<2,3>", 64, 64, 3, 24),
    C("k_conv_bx<4,1>", 64, 128, 1, 8),
    C("k_conv_bx<4,3>", 64, 128, 3, 24),                # odd tiles_x keeps the 8 x 8 tile
    C("k_conv_bx<4,3>", 128, 128, 3, 4, up=True),
    C("k_conv_bx<4,3,4>", 64, 128, 3, 16),
    C("k_conv_bx<4,3,4>", 128, 128, 3, 8, up=True),
    C("k_conv_bx<4,3,4>", 96, 128, 3, 16),              # three rounds: the register ring across round boundaries
    C("k_conv_bx<4,3,2,2>", 32, 128, 3, 16, stride=2),
    C("k_conv_bx<4,3,2,2>", 64, 128, 3, 16, stride=2),
    C("k_conv_few<3>", 32, 3, 3, 16, res=False),        # a residual would move the conv off k_conv_few
    C("k_conv_few<3>", 32, 3, 3, 32, res=False),
    C("k_conv_few<4>", 32, 4, 3, 16, res=False),
    C("k_conv_few<4>", 32, 4, 3, 32, res=False),
]
_ids = [c.id for c in CONV_CASES]


@pytest.mark.parametrize("case", CONV_CASES, ids=_ids)
def test_conv_impulse_response(case):
    K.check_impulse(case)


@pytest.mark.parametrize("case", CONV_CASES, ids=_ids)
def test_conv_dense_within_twice_an_fp32_chain(case):
    K.check_dense(case)


@pytest.mark.parametrize("case", CONV_CASES, ids=_ids)
def test_conv_epilogue_is_exact(case):
    K.check_epilogue(case)


@pytest.mark.parametrize("case", [c for c in CONV_CASES if c.cin % 8], ids=[c.id for c in CONV_CASES if c.cin % 8])
def test_conv_ignores_input_padding_channels(case):
    K.check_input_padding(case)


# ------------------------------------------------------------------------------------------------ fused GroupNorm
# 3 x 3 identity conv C -> C: the instantiation depends on C only at these sizes (8 x 8: one tile; 24 x 24: odd tiles_x)
GN_KERNEL = {32: "k_conv_bx<1,3>", 64: "k_conv_bx<2,3>", 96: "k_conv_bx<2,3>", 128: "k_conv_bx<4,3>", 256: "k_conv_bx<4,3>"}


@pytest.mark.parametrize("swish", [0, 1])
@pytest.mark.parametrize("hw", [8, 24])                 # 64 pixels: one chunk in k_gn_partial; 576: two
@pytest.mark.parametrize("Cc", [32, 64, 96, 128, 256])  # 1, 2, 3 (a float4 straddles two groups), 4 and 8 channels per group
def test_fused_groupnorm_stages_the_normalised_activation(Cc, hw, swish):
    K.check_fused_gn_identity(GN_KERNEL[Cc], Cc, hw, swish)


def test_fused_groupnorm_with_group_means_a_thousand_sigmas_out():
    K.check_fused_gn_identity(GN_KERNEL[128], 128, 8, 1, offset_sigmas=1000.0)


@pytest.mark.parametrize("Cc,cout,kernel", [(32, 32, "k_conv_bx<1,3>"), (64, 64, "k_conv_bx<2,3>"), (96, 128, "k_conv_bx<4,3,4>"),
                                             (128, 128, "k_conv_bx<4,3,4>"), (256, 128, "k_conv_bx<4,3,4>")])
def test_dense_conv_behind_a_fused_groupnorm(Cc, cout, kernel):
    K.check_fused_gn_dense(kernel, Cc, cout, 16)


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("hw", [8, 24])                 # 1 tile; 9 tiles: k_gn_finalize_tiles wraps its 8 partial sums
@pytest.mark.parametrize("cout", [128, 256, 512])       # 4, 8, 16 channels per group
@pytest.mark.parametrize("kernel,cin,ks", [("k_conv<4>", 3, 3), ("k_conv_bx<4,1>", 64, 1), ("k_conv_bx<4,3>", 32, 3)])
def test_output_statistics_both_paths(kernel, cin, ks, cout, hw):
    for with_res in (False, True):
        K.check_stats(kernel, cin, cout, ks, hw, with_res)


@pytest.mark.parametrize("hw", [(8, 16), (40, 16)])     # the wide kernel needs an even tiles_x: 2 tiles, and 10 (wraps the 8 sums)
@pytest.mark.parametrize("cout", [128, 256, 512])
def test_output_statistics_both_paths_wide_kernel(cout, hw):
    for with_res in (False, True):
        K.check_stats("k_conv_bx<4,3,4>", 32, cout, 3, hw, with_res)


@pytest.mark.parametrize("hw", [8, 24])
def test_output_statistics_three_channels_per_group(hw):
    """C = 96 never qualifies for the epilogue statistics: k_gn_partial + k_gn_finalize whether the tracker is armed or not."""
    for with_res in (False, True):
        K.check_stats("k_conv_bx<2,3>", 32, 96, 3, hw, with_res)


# ------------------------------------------------------------------------------------------------ attention core
@pytest.mark.parametrize("N,Cc,hw,path,kernels", [
    (64, 64, 8, "bf16_pipe", ("k_conv_bx<2,1>", "k_conv_bx<2,1>")),
    (256, 128, 16, "bf16_pipe", ("k_conv_bx<4,1>", "k_conv_bx<4,1>")),
    (64, 32, 8, "scalar", ("k_attn_scores", "k_attn_pv"))])
def test_attention_core(N, Cc, hw, path, kernels):
    K.check_attention(N, Cc, hw, path, kernels)


# ------------------------------------------------------------------------------------------------ nearest-code search
# (P, E, N) -> what run_vq_argmin launches.  Code splits double while 2 * splits * pixel groups fit 256 CUs and every wave keeps a
# 32-code tile: 512 codes in one pixel group split 4 ways, 128 codes are the one-split case.
ARGMIN_CASES = [(64, 8, 128, "k_vq_argmin"),
                (192, 64, 1024, "k_vq_argmin_split<4> (8 code splits)"),      # a half-empty last pixel group
                (128, 256, 512, "k_vq_argmin_split<4> (4 code splits)"),
                (128, 256, 128, "k_vq_argmin_split<4> (1 code splits)")]


@pytest.mark.parametrize("P,E,N,path", ARGMIN_CASES)
def test_nearest_code_search(P, E, N, path):
    K.check_argmin(P, E, N, path)


_CHILD_HEAD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from tests import vq_layer_checks as K
from tests.vq_layer_checks import ConvCase as C
"""

_CHILD_NO_SPLIT = _CHILD_HEAD + r"""
out = {}
for P, E, N in %r:
    out["%%d_%%d_%%d" %% (P, E, N)] = K.check_argmin(P, E, N, "k_vq_argmin")
np.savez(sys.argv[1], **out)
"""

_CHILD_NO_BX = _CHILD_HEAD + r"""
for case in (C("k_conv<4>", 32, 128, 3, 16), C("k_conv<4>", 64, 128, 1, 16)):      # full rounds: double-buffered staging
    K.check_impulse(case)
    K.check_dense(case)
    K.check_epilogue(case)
    K.check_fused_gn_dense("k_conv<4>", case.cin, 128, 16, ks=case.ks)
for swish in (0, 1):
    K.check_fused_gn_identity("k_conv<4>", 128, 8, swish)
    K.check_fused_gn_identity("k_conv<2>", 96, 8, swish)          # three channels per group through conv_gn in the fp32 kernel
K.check_attention(64, 64, 8, "scalar", ("k_attn_scores", "k_attn_pv"))
print("CHILD OK")
"""


def _child(script, env_extra, *argv):
    res = subprocess.run([sys.executable, "-c", script, *argv], env=dict(os.environ, **env_extra), capture_output=True, text=True,
                         timeout=300, cwd=REPO)
    print(res.stdout)
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-2500:])
    return res.stdout


def test_split_search_is_bit_identical_to_the_unsplit_kernel(tmp_path):
    """The same inputs with WMAR_VQ_NO_SPLIT=1 (read once per process: a child): k_vq_argmin must pass the same checks and return the
    same code for every pixel as k_vq_argmin_split."""
    shapes = [(P, E, N) for P, E, N, path in ARGMIN_CASES if "split" in path]
    out = tmp_path / "codes.npz"
    _child(_CHILD_NO_SPLIT % (REPO, shapes), {"WMAR_VQ_NO_SPLIT": "1"}, str(out))
    old = np.load(out)
    for P, E, N, path in ARGMIN_CASES:
        if "split" in path:
            assert np.array_equal(K.check_argmin(P, E, N, path), old["%d_%d_%d" % (P, E, N)]), (P, E, N)


def test_fp32_opt_out_convolutions_and_attention():
    """WMAR_CONV_NO_BX=1 (the opt-out for models with non-finite activations, read once per process: a child): k_conv<4> with
    double-buffered staging, with and without fused GroupNorm, and the scalar attention kernels at a shape the bf16 pipe would take."""
    assert "CHILD OK" in _child(_CHILD_NO_BX % REPO, {"WMAR_CONV_NO_BX": "1"})
