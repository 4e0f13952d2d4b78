"""The VQGAN layer plans (wmar_amd/csrc/vq_plan.h) on the CPU: tests/vq_plan_dump.cpp, built with the host compiler, prints the plan of a config;
the checkpoint tensors it names, the safety of its inference slots, its memory footprint and the order inside its blocks are checked here."""
import functools
import os
import subprocess
from collections import namedtuple

import pytest

from tests.conftest import REPO

GN, CONV, ATTN, POOL = 0, 1, 2, 3
Op = namedtuple("Op", "half kind inp out res conv norm swish up q k v")
Conv = namedtuple("Conv", "name cin cout ks stride bias")
Tensor = namedtuple("Tensor", "C H slot")
Plan = namedtuple("Plan", "resolution S in_channels out_ch unit_range max_batch rot_elems att_elems max_elems attn_nn zbias_elems "
                          "tensors norms convs halves ops")


def _configs():
    from wmar_amd.utils import synth
    return {
        "harness": synth.VQConfig(**synth.HARNESS_VQ),
        "wide": synth.VQConfig(ch=64, ch_mult=(1, 2), num_res_blocks=2, attn_resolutions=(16,), resolution=32, z_channels=16, embed_dim=8,
                               n_embed=512),                                                               # test_gpu_vq_train.py
        "taming": synth.TAMING_VQ,
        "chameleon": synth.CHAMELEON_VQ,
        "maskgit": synth.MASKGIT_VQ,
        "mvq_small": synth.MaskgitVQConfig(hidden_channels=32, channel_mult=(1, 2, 2), num_res_blocks=1, resolution=32, z_channels=16,
                                           num_embeddings=512),                                            # test_gpu_mvq_train.py
        "mvq_wide": synth.MaskgitVQConfig(hidden_channels=64, channel_mult=(1, 1, 2), num_res_blocks=2, resolution=32, z_channels=32,
                                          num_embeddings=512),
    }


NAMES = ["harness", "wide", "taming", "chameleon", "maskgit", "mvq_small", "mvq_wide"]


def _is_mvq(cfg):
    return hasattr(cfg, "hidden_channels")


def dump_args(cfg, max_batch=2):
    """The command line of vq_plan_dump for a synth config."""
    csv = lambda xs: ",".join(str(x) for x in xs)
    if _is_mvq(cfg):
        return ["mvq"] + [str(x) for x in (cfg.hidden_channels, cfg.num_res_blocks, cfg.resolution, cfg.num_channels, cfg.z_channels,
                                           cfg.num_embeddings, max_batch)] + [csv(cfg.channel_mult)]
    a = ["taming"] + [str(x) for x in (cfg.ch, cfg.num_res_blocks, cfg.resolution, cfg.in_channels, cfg.out_ch, cfg.z_channels, cfg.embed_dim,
                                       cfg.n_embed, max_batch)] + [csv(cfg.ch_mult)]
    return a + ([csv(cfg.attn_resolutions)] if cfg.attn_resolutions else [])


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """name -> Plan, through the dump program built once with the host compiler."""
    exe = str(tmp_path_factory.mktemp("vq_plan") / "vq_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", os.path.join(REPO, "tests", "vq_plan_dump.cpp"), "-o", exe])
    return functools.lru_cache(maxsize=None)(lambda name: _parse(subprocess.check_output([exe] + dump_args(_configs()[name])).decode()))


def _parse(text):
    head, tensors, norms, convs, halves, ops = None, [], [], [], {}, {0: [], 1: []}
    for line in text.splitlines():
        f = line.split()
        if f[0] == "plan":
            head = [int(x) for x in f[1:]]
        elif f[0] == "tensor":
            assert int(f[1]) == len(tensors)
            tensors.append(Tensor(*(int(x) for x in f[2:])))
        elif f[0] == "norm":
            assert int(f[1]) == len(norms)
            norms.append((f[2], int(f[3])))
        elif f[0] == "conv":
            assert int(f[1]) == len(convs)
            convs.append(Conv(f[2], *(int(x) for x in f[3:])))
        elif f[0] == "half":
            halves[int(f[1])] = (int(f[2]), int(f[3]))
        elif f[0] == "op":
            o = Op(*(int(x) for x in f[1:]))
            ops[o.half].append(o)
        else:
            raise AssertionError(line)
    return Plan(*head, tensors, norms, convs, halves, ops)


def _reads(o):
    if o.kind == ATTN:
        return [o.q, o.k, o.v]
    return [t for t in (o.inp, o.res) if t >= 0]


@pytest.mark.parametrize("name", NAMES)
def test_plan_names_every_checkpoint_tensor_with_its_shape(name, plans):
    """The (name.weight, name.bias) tensors of the plan's convs and norms == the checkpoint layout minus the codebook; bias-free convs have
    no .bias entry.  Every conv and every norm is used by exactly one CONV / GN op."""
    from wmar_amd.utils import synth
    cfg, p = _configs()[name], plans(name)
    want = dict(synth.maskgit_shapes(cfg) if _is_mvq(cfg) else synth.vq_shapes(cfg))
    del want["quantize.embedding.weight"]
    got = {}
    for n, C in p.norms:
        got[n + ".weight"] = (C,)
        got[n + ".bias"] = (C,)
    for c in p.convs:
        got[c.name + ".weight"] = (c.cout, c.cin, c.ks, c.ks)
        if c.bias:
            got[c.name + ".bias"] = (c.cout,)
    assert len(got) == 2 * len(p.norms) + len(p.convs) + sum(c.bias for c in p.convs), "a name appears twice"
    assert got == {k: tuple(v) for k, v in want.items()}
    ops = p.ops[0] + p.ops[1]
    assert sorted(o.conv for o in ops if o.kind == CONV) == list(range(len(p.convs)))
    assert sorted(o.norm for o in ops if o.kind == GN) == list(range(len(p.norms)))


@pytest.mark.parametrize("name", NAMES)
def test_no_op_overwrites_a_slot_that_is_still_read(name, plans):
    """Walking each half in order with the inference slots: whatever an op reads is still in its slot, no op writes a slot whose tensor a
    later op (or the caller: the half's last tensor) reads, and an op's in, res and out are distinct slots unless in == res (the MaskGIT
    shortcut nin(h) + h).  Shapes follow the ops, and a conv that applies a norm follows the GN op of that norm on the same tensor."""
    p = plans(name)
    for h in (0, 1):
        ops = p.ops[h]
        first, last = p.halves[h]
        last_use = {last: len(ops)}
        for i, o in enumerate(ops):
            for t in _reads(o):
                last_use[t] = max(last_use.get(t, -1), i)
        holder = {p.tensors[first].slot: first}
        stats_of = {}                                    # norm -> the tensor its statistics describe
        for i, o in enumerate(ops):
            for t in _reads(o):
                assert holder.get(p.tensors[t].slot) == t, (h, i, "reads a tensor that is no longer in its slot")
            x = p.tensors[o.inp]
            if o.kind == GN:
                assert x.C == p.norms[o.norm][1]
                stats_of[o.norm] = o.inp
                continue
            y = p.tensors[o.out]
            if o.kind == CONV:
                c = p.convs[o.conv]
                assert x.C == (c.cin + 7) // 8 * 8 and y.C == (c.cout + 7) // 8 * 8
                assert y.H == (2 * x.H if o.up else x.H // 2 if c.stride == 2 else x.H)
                assert not (o.up and c.stride == 2)
                if o.norm >= 0:
                    assert stats_of.get(o.norm) == o.inp and not o.up
                if o.res >= 0:
                    assert p.tensors[o.res][:2] == y[:2]
                slots = [p.tensors[t].slot for t in {o.inp, o.res} if t >= 0] + [y.slot]
                assert len(set(slots)) == len(slots), (h, i, "in, res and out share a slot")
            elif o.kind == POOL:
                assert (y.C, y.H) == (x.C, x.H // 2) and y.slot != x.slot
            else:
                q = p.tensors[o.q]
                assert all(p.tensors[t][:2] == q[:2] for t in (o.k, o.v, o.out))
                assert len({p.tensors[t].slot for t in (o.q, o.k, o.v, o.out)}) == 4
            prev = holder.get(y.slot)
            assert prev is None or last_use.get(prev, -1) < i, (h, i, "overwrites a tensor that is still read")
            holder[y.slot] = o.out
        assert holder[p.tensors[last].slot] == last


def _parent_maxel(cfg):
    """Elements per image of one rotating buffer as the engines sized it before the plan existed (their create functions' formulas)."""
    pad8 = lambda c: (c + 7) // 8 * 8
    if _is_mvq(cfg):
        ch, mult, z = cfg.hidden_channels, cfg.channel_mult, cfg.z_channels
    else:
        ch, mult, z = cfg.ch, cfg.ch_mult, None
    L, r, maxel = len(mult), cfg.resolution, 0
    for lvl in range(L):
        cmax = ch * mult[lvl]
        if lvl > 0:
            cmax = max(cmax, ch * mult[lvl - 1])
        if lvl + 1 < L:
            cmax = max(cmax, ch * mult[lvl + 1])
        if z is not None and lvl == L - 1:
            cmax = max(cmax, z)
        maxel = max(maxel, r * r * pad8(cmax))
        r //= 2
    if z is None:
        maxel = max(maxel, cfg.resolution ** 2 * pad8(max(cfg.in_channels, cfg.out_ch)))
    return maxel


@pytest.mark.parametrize("name", NAMES)
def test_footprint_is_within_what_the_engines_allocated_before(name, plans):
    """At most four rotating slots plus the four attention tensors; every tensor fits the buffer of its slot; a rotating buffer is no
    larger than the formula the engines used, the attention buffers no larger than max tokens x max channels (x max tokens)."""
    cfg, p = _configs()[name], plans(name)
    assert {t.slot for t in p.tensors} <= set(range(8))
    attn_ops = [o for o in p.ops[0] + p.ops[1] if o.kind == ATTN]
    for o in p.ops[0] + p.ops[1]:
        if o.kind == ATTN:
            assert [p.tensors[t].slot for t in (o.q, o.k, o.v, o.out)] == [4, 5, 6, 7]
    att = {t for o in attn_ops for t in (o.q, o.k, o.v, o.out)}
    for i, t in enumerate(p.tensors):
        assert (t.slot >= 4) == (i in att)
        assert t.C * t.H * t.H <= (p.att_elems if t.slot >= 4 else p.rot_elems) <= p.max_elems
    assert p.rot_elems <= _parent_maxel(cfg)
    assert (p.resolution, p.S) == (cfg.resolution, cfg.codes_size) and p.unit_range == _is_mvq(cfg)
    if _is_mvq(cfg):
        assert not attn_ops and p.att_elems == 0 and p.attn_nn == 0
        assert p.in_channels == p.out_ch == cfg.num_channels
    else:
        ntok = max(list(cfg.attn_resolutions) + [cfg.codes_size]) ** 2
        cam = cfg.ch * max(cfg.ch_mult)
        assert p.att_elems <= ntok * cam and p.attn_nn <= ntok * ntok and p.zbias_elems == max(ntok, cam)
        assert all(p.tensors[o.q].H ** 2 <= p.zbias_elems and p.tensors[o.q].C <= p.zbias_elems for o in attn_ops)
        assert p.attn_nn == max(p.tensors[o.q].H ** 4 for o in attn_ops)
        assert (p.in_channels, p.out_ch) == (cfg.in_channels, cfg.out_ch)


def _blocks(p, h):
    """The ops of a half grouped by the block that owns them: prefix -> [(label, op)], label = gn:<norm leaf> | <conv leaf> | attn | pool."""
    out, cur = {}, None
    for o in p.ops[h]:
        if o.kind == GN:
            name = p.norms[o.norm][0]
            cur, label = name.rpartition(".")[0], "gn:" + name.rpartition(".")[2]
        elif o.kind == CONV:
            name = p.convs[o.conv].name
            cur, label = name.rpartition(".")[0], name.rpartition(".")[2]
        elif o.kind == ATTN:
            label = "attn"                               # between its block's v and proj_out
        else:
            cur, label = "pool%d" % len(out), "pool"
        out.setdefault(cur, []).append((label, o))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_order_inside_the_blocks(name, plans):
    """Taming ResnetBlock: gn, conv1, gn, [nin_shortcut of the block input,] conv2(res = shortcut).  MaskGIT: gn, conv1, gn, conv2,
    [nin_shortcut(in = res = h)].  AttnBlock: gn, q, k, v, attn, proj_out(res = x)."""
    cfg, p = _configs()[name], plans(name)
    seen = set()
    for h in (0, 1):
        for prefix, ops in _blocks(p, h).items():
            labels = [l for l, _ in ops]
            o = [x for _, x in ops]
            if labels[0] == "gn:norm1":
                X = o[0].inp
                cin, cout = p.convs[o[1].conv].cin, p.convs[o[1].conv].cout
                assert (o[1].inp, o[1].norm, o[1].swish, o[1].res) == (X, o[0].norm, 1, -1) and o[0].swish == 1
                assert (o[2].inp, o[2].swish) == (o[1].out, 1)
                if _is_mvq(cfg):
                    assert labels == ["gn:norm1", "conv1", "gn:norm2", "conv2"] + (["nin_shortcut"] if cin != cout else [])
                    assert (o[3].inp, o[3].norm, o[3].swish) == (o[1].out, o[2].norm, 1)
                    if cin != cout:
                        assert o[3].res == -1 and (o[4].inp, o[4].res, o[4].norm) == (o[3].out, o[3].out, -1)
                        assert (p.convs[o[4].conv].cin, p.convs[o[4].conv].cout, p.convs[o[4].conv].ks) == (cout, cout, 1)
                    else:
                        assert o[3].res == X
                    assert not any(p.convs[x.conv].bias for x in o if x.kind == CONV)
                else:
                    assert labels == ["gn:norm1", "conv1", "gn:norm2"] + (["nin_shortcut"] if cin != cout else []) + ["conv2"]
                    if cin != cout:
                        assert (o[3].inp, o[3].res, o[3].norm) == (X, -1, -1)
                        assert (p.convs[o[3].conv].cin, p.convs[o[3].conv].cout, p.convs[o[3].conv].ks) == (cin, cout, 1)
                    assert (o[-1].inp, o[-1].norm, o[-1].swish) == (o[1].out, o[2].norm, 1)
                    assert o[-1].res == (o[3].out if cin != cout else X)
                seen.add("res_nin" if cin != cout else "res")
            elif labels[0] == "gn:norm":
                assert labels == ["gn:norm", "q", "k", "v", "attn", "proj_out"]
                X = o[0].inp
                assert o[0].swish == 0 and all((x.inp, x.norm, x.swish, x.res) == (X, o[0].norm, 0, -1) for x in o[1:4])
                assert (o[4].q, o[4].k, o[4].v) == (o[1].out, o[2].out, o[3].out)
                assert (o[5].inp, o[5].res, o[5].norm) == (o[4].out, X, -1)
                seen.add("attn")
    assert "res" in seen and ("attn" in seen) == (not _is_mvq(cfg))
    assert "res_nin" in seen                             # every config here changes the channel count somewhere
