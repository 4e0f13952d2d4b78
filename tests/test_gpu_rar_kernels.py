"""The launches of one RAR position one at a time, through a live engine's own RarPlan and buffers (wmar_rar_probe_run /
wmar_rar_probe_copy / wmar_rar_probe_plan), against the numpy statement of that one operation in tests/rar_kernel_reference.py.
Every case asserts the kernel names and integers of the probe plan against the dispatch rules written down a second time
(rar_kernel_reference.expected_plan) and the facts pinned in HEADLINE, and prints its figures on lines starting RARK (run with -s).

Engines (synthetic weights from numpy; image_seq_len 16 = 18 positions unless the SHAPES entry names another (Probe.SEQ / Probe.T),
vocabulary 256, 8 classes, max_batch 64 = up to 128 rows; "int": integer weights, embeddings and biases, LayerNorm weights powers of
two; "dense": full-significand).  SHAPES also holds the engines of tests/test_gpu_rar_released.py, which runs this file's bodies at the
released widths; the cases of this file use R1 .. R7:
  R1  128 wide, 4 heads of 32, F 512, 2 blocks    the fp32-MFMA plan at 1 / 2 / 4 row tiles, k_resid_mod<S, 1>
  R2  320 wide, 4 heads of 80, F 1280, 2 blocks   k_bx at PER 5 / 5 / 4 with S 1 / 1 / 5 above 64 rows, row-major QKV pieces into
                                                  k_attn_decode80; packed pieces below 65 rows and with WMAR_NO_BX=1
  R3  1280 wide, 16 heads of 80, F 5120, 1 block  k_bx<4,20,2> adaLN at 33..64 adaLN rows, the XF GELU FC1, production PER / S
  R4  2176 wide, 17 heads of 128, F 2176, 1 block KPW = 4 k_resid_mod (17 chunks), 17 statistics chunks in k_modulate / k_rar_embed
  R5 / R6 / R7  352 wide, 4 heads of 88 / 192 wide, 4 heads of 48 / 128 wide, 2 heads of 64, one block each

What is asserted
  exact (0 differing bits): the embedding's x and its fp64 statistics on integer embeddings; the gated fold on integer operands with
      power-of-two gates and the partial sums it publishes; one-hot attention; every work buffer a RESID_*, MOD_IN or ATTN launch does
      not own, byte for byte; cache rows below the position and other rows'
      caches; padding rows of sc / mod past the adaLN row tiles; the bf16 planes as the split of their own sum.
  exact between paths: RESID_ATTN / RESID_MLP fused against the two-launch pair (WMAR_NO_XR=1 engine, same inputs copied in): x, h /
      planes and part; a shared_u walk against a plain walk whose `mod` rows of the unconditional half hold the table's row of the
      position, with 3e30 in every table row and `mod` row the shared_u walk must not read; the stage walk over sentinel-filled
      work buffers against wmar_rar_forward_position: logits and cache bits.
  held to float64: SiLU rows (7 x 2^-24 of the value, derived), k_modulate / k_resid_mod outputs per element to the normaliser rule of
      rar_kernel_reference.modulate64 (none exempt), the dense gated fold, the appended q-normed / k-normed rows (2 x the fp32
      algebra), dense attention (the derived distance per output, 4 x an fp32 numpy evaluation per launch), the unconditional table
      (DENSE_GATE = 2 x the fp32 chain plus the SiLU distance), the dense QKV / PROJ / FC2 pieces and the head (the chain bound), the dense adaLN GEMM (k_gemm and k_bx<4,20,2>) and the dense FC1 through its GELU (k_gemm, planes, the XF k_bx).
Row counts of the stage-level groups: R1 at 1 / 5 / 31 / 32 / 33 / 63 / 64 / 65 / 127 / 128 (not every group has all ten), Bhalf 31 / 32 / 33 / 63 / 64.
A launch that fails on the device ends the session (tests/engine_probe.py: EngineProbe._checked); nothing is retried.

Measured on an MI355X (365 cases, 35 s): 0 differing bits in every exact and between-paths case, 0 bytes changed in buffers a launch
does not own; SiLU 0.15 .. 0.35 of its distance (an fp32 numpy evaluation 0.25 .. 0.49); k_modulate 0.56 .. 0.96 and k_resid_mod 0.44 ..
0.98 of the per-element distance (fp32 numpy 0.42 .. 0.98: the final addition's half ulp fills it where the shift dominates); dense gated
fold <= 0.98; appended k rows 0.02 .. 0.61 of the derived distance and 1.00 .. 1.32 x the fp32 algebra (gate 2); dense attention <= 0.007
of the derived distance, 0 .. 2.03 x the fp32 evaluation (gate 4); table 0.24 .. 0.38 x the chain; dense pieces 0.22 .. 0.55 x, adaLN GEMM
0.26 .. 0.43 x (k_bx<4,20,2>: 0.26) and head 0.30 .. 0.47 x the chain (gate 2); GELU 0.25 of its distance on exact pre-activations, 0.06 ..
0.16 on dense ones (XF k_bx: 0.06 .. 0.08).  DESIGN.md section 4 has the table."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import rar_kernel_reference as R  # noqa: E402
from tests.engine_probe import EngineCache, EngineProbe, dev, parse_plan, say  # noqa: E402

SENT = float(R.SENTINEL)
GARBAGE = 3.0e30
V, NCLS = 256, 8
SEQ_DEFAULT = 16                  # image_seq_len of an engine whose SHAPES entry names none: T = 18 positions
NONE_ID = NCLS + V + 1
WORK = ["x", "h", "y", "sc", "hbuf", "slabs", "qkv_slabs", "mod", "xq", "yq", "hq", "scq"]

SHAPES = {  # name: (D, H, F, L, max_batch[, image_seq_len])
    "R1": (128, 4, 512, 2, 64), "R2": (320, 4, 1280, 2, 64), "R3": (1280, 16, 5120, 1, 64), "R4": (2176, 17, 2176, 1, 64),
    "R5": (352, 4, 704, 1, 64), "R6": (192, 4, 384, 1, 64), "R7": (128, 2, 256, 1, 64),
}
# the engines of tests/test_gpu_rar_released.py (which runs the bodies of this file on them): one block of a released width, the
# two k_bx<2,16,4> / <2,20,4> shapes, and narrow engines of 258 positions for the attention launch alone
SHAPES.update({n: (D, H, F, 1, 64) for n, (D, H, F) in R.RELEASED_SHAPES.items() if n != "RXL"})
SHAPES.update({"A%d" % hd: (4 * hd, 4, 8 * hd, 1, 32, 256) for hd in (32, 48, 64, 80, 88, 128)})
SHAPES["A80R"] = (320, 4, 1280, 1, 64, 256)
# facts the issue names per engine; checked on top of expected_plan (which restates the whole dispatch)
HEADLINE = {
    ("R2", 128): dict(bx=1, rowmajor=1, PER_qkv=5, S_qkv=1, PER_proj=5, S_proj=1, S_fc2=5),
    ("R2", 64): dict(bx=0, rowmajor=0),
    ("R3", 128): dict(bx=1, fc1_bx=1, S_qkv=4, PER_qkv=5, S_proj=5, PER_proj=4, S_fc2=8, PER_fc2=10),
    ("R4", 5): dict(kpw=4, nrm=17, nch=17), ("R4", 128): dict(kpw=4, nrm=17, nch=17, bx=0),
    ("R1", 5): dict(kpw=1, nrm=4, bx=0), ("R1", 128): dict(kpw=1, nrm=4, bx=0, MT=4),
    ("A80R", 128): dict(bx=1, rowmajor=1, S_qkv=1, roles=dict(attn="k_attn_decode80<1> rowmajor")),
}
HEADLINE.update({k: v for k, v in R.released_pins().items() if k[0] in SHAPES})


_say = say("RARK", 44)


def _shapes(D, H, F, L, SEQ):
    hd = D // H
    s = {"cls_token": (1, 1, D)}
    for i in range(L):
        p = "blocks.%d." % i
        s.update({p + "norm1.weight": (D,), p + "norm1.bias": (D,), p + "attn.qkv.weight": (3 * D, D), p + "attn.qkv.bias": (3 * D,),
                  p + "attn.q_norm.weight": (hd,), p + "attn.q_norm.bias": (hd,), p + "attn.k_norm.weight": (hd,), p + "attn.k_norm.bias": (hd,),
                  p + "attn.proj.weight": (D, D), p + "attn.proj.bias": (D,), p + "norm2.weight": (D,), p + "norm2.bias": (D,),
                  p + "mlp.fc1.weight": (F, D), p + "mlp.fc1.bias": (F,), p + "mlp.fc2.weight": (D, F), p + "mlp.fc2.bias": (D,),
                  p + "adaLN_modulation.1.weight": (6 * D, D), p + "adaLN_modulation.1.bias": (6 * D,)})
    s.update({"embeddings.weight": (V + 1 + NCLS + 1, D), "pos_embed": (1, SEQ + 1024, D), "target_aware_pos_embed": (1, SEQ + 1024, D),
              "timesteps_embeddings": (1, SEQ + 100, D), "adaln_before_head.adaLN_modulation.1.weight": (2 * D, D),
              "adaln_before_head.adaLN_modulation.1.bias": (2 * D,), "lm_head.weight": (V, D), "lm_head.bias": (V,)})
    return s


def _shape_of(name):
    """(D, H, F, L, max_batch, image_seq_len) of an engine"""
    return (tuple(SHAPES[name]) + (SEQ_DEFAULT,))[:6]


def _state(name, kind):
    D, H, F, L, _, SEQ = _shape_of(name)
    T = SEQ + 2
    rng = np.random.default_rng(1000 + D + (7 if kind == "int" else 0))
    sd = {}
    for k, shp in _shapes(D, H, F, L, SEQ).items():
        leaf = k.rsplit(".", 1)[-1]
        norm = "norm" in k
        if kind == "int":
            if norm:
                v = 2.0 ** rng.integers(-1, 2, size=shp) if leaf == "weight" else rng.integers(-2, 3, size=shp) * 0.5
            elif k in ("pos_embed", "target_aware_pos_embed", "timesteps_embeddings"):
                v = rng.integers(-4, 5, size=(1, T + 2, shp[2]))
            else:
                v = rng.integers(-4, 5, size=shp) if leaf != "bias" else rng.integers(-2, 3, size=shp)
        else:
            if norm:
                v = rng.standard_normal(shp, dtype=np.float32) * 0.1 + (1.0 if leaf == "weight" else 0.0)
            elif k in ("pos_embed", "target_aware_pos_embed", "timesteps_embeddings"):
                v = rng.standard_normal((1, T + 2, shp[2]), dtype=np.float32) * 0.5
            elif k in ("embeddings.weight", "cls_token"):
                v = rng.standard_normal(shp, dtype=np.float32)
            elif leaf == "bias":
                v = rng.standard_normal(shp, dtype=np.float32) * 0.1
            else:
                v = rng.standard_normal(shp, dtype=np.float32) * (1.0 / np.sqrt(shp[-1]))
        v = np.asarray(v, dtype=np.float32)
        if k in ("pos_embed", "target_aware_pos_embed", "timesteps_embeddings"):       # only the first T + 2 rows are ever read
            full = np.zeros(shp, dtype=np.float32)
            full[:, :T + 2] = v
            v = full
        sd[k] = v
    return sd


class Probe(EngineProbe):
    """One wmar_rar engine and stage access to it."""
    ENGINE = "rar"
    DTYPES = {"stats": torch.float64, "part": torch.int64, "ids": torch.int64, "cond_ids": torch.int64, "ctr": torch.int32,
              "xq": torch.int16, "yq": torch.int16, "hq": torch.int16, "scq": torch.int16}
    U64 = {"part"}

    def __init__(self, name, kind, env=()):
        self.name, self.kind, self.env = name, kind, env
        self.D, self.H, self.F, self.nl, self.Bmax, self.SEQ = _shape_of(name)
        self.T = self.SEQ + 2
        self.hd, self.Ntot, self.Mmax = self.D // self.H, 6 * self.D * self.nl + 2 * self.D, 2 * self.Bmax
        self.MTmax = R.mt_for(self.Mmax)
        self.sd = _state(name, kind)
        from wmar_amd import _lib
        self._create(_lib.RarConfig(self.D, self.nl, self.H, self.F, self.SEQ, V, NCLS, self.Bmax), self.sd, env)
        self.wada = np.concatenate([self.sd["blocks.%d.adaLN_modulation.1.weight" % i] for i in range(self.nl)] + [self.sd["adaln_before_head.adaLN_modulation.1.weight"]])
        self.bada = np.concatenate([self.sd["blocks.%d.adaLN_modulation.1.bias" % i] for i in range(self.nl)] + [self.sd["adaln_before_head.adaLN_modulation.1.bias"]])

    def sentinel_work(self):
        for nme in WORK:
            if self.has(nme):
                if self._dt(nme) == torch.int16:
                    self.fill(nme, 0x7f7f)
                else:
                    self.fill(nme, SENT)
        self.fill("stats", 1e300)

    def snapshot(self):
        """device copies of every work buffer, the statistics and the partial sums, taken in front of a launch"""
        return {n: self.get_dev(n).clone() for n in WORK + ["stats", "part"] if self.has(n)}

    def assert_unowned_unchanged(self, snap, owned, part_words=None):
        """every buffer outside `owned` holds the bytes of the snapshot; part_words = (first, end): the u64 words of `part` the launch owns"""
        for n, before in snap.items():
            if n in owned:
                continue
            now = self.get_dev(n)
            if n == "part" and part_words is not None:
                now, before = now.clone(), before.clone()
                now[part_words[0]:part_words[1]] = 0
                before[part_words[0]:part_words[1]] = 0
            assert torch.equal(now.view(torch.uint8), before.view(torch.uint8)), "%s: a buffer the launch does not own changed" % n

    # ---- stages
    def run(self, first, last, M, Bhalf=None, shared_u=0, pos=0, layer=0, tok=None, cond=None, want_logits=False):
        Bhalf = M if Bhalf is None else Bhalf
        return self._call(self._run, M, V, dev(tok), dev(cond), M, Bhalf, shared_u, pos, layer, first, last, want_logits=want_logits)

    def walk(self, M, Bhalf, shared_u, pos, first=R.EMBED, tok=None, cond=None):
        """the position from stage `first` (of block 0) to HEAD, one probe call per block"""
        if first <= R.MOD_IN:
            self.run(first, R.MOD_IN, M, Bhalf, shared_u, pos, 0, tok, cond)
            first = R.QKV
        for l in range(self.nl):
            self.run(first if l == 0 else R.QKV, R.RESID_MLP, M, Bhalf, shared_u, pos, l)
        return self.run(R.HEAD, R.HEAD, M, Bhalf, shared_u, pos, self.nl - 1, want_logits=True)

    def forward_position(self, tok, cond, pos):
        return self._call(self.L.wmar_rar_forward_position, len(tok), V, dev(tok), dev(cond), len(tok), pos)

    def plan(self, M, Bhalf=None, shared_u=0, kv_len=1):
        """the plan for M rows, held to the restated dispatch rules and the pinned facts: a shape that silently takes another path fails"""
        Bhalf = M if Bhalf is None else Bhalf
        out = parse_plan(self.plan_text(M, Bhalf, shared_u, kv_len))
        assert all(isinstance(v, int) for k, v in out.items() if k not in ("stages", "kernels", "roles")), out
        want = R.expected_plan(self.D, self.H, self.F, self.nl, V, self.Bmax, M, Bhalf, shared_u, no_bx="WMAR_NO_BX" in self.env,
                               fused="WMAR_NO_XR" not in self.env)
        assert out["fallbacks"] == 0, "an in-launch wait gave up: the engine left the fused launch"
        for k, v in want.items():
            assert out[k] == v, (self.name, M, k, out[k], v)
        R.check_pins(out, HEADLINE.get((self.name, M), {}) if not self.env else {}, (self.name, M))
        return out

    # ---- packed buffers as [rows, width] arrays
    def put_act(self, name, X, MT, rest=None):
        self.put_front(name, R.pack_rows(X.astype(np.float32), MT), rest=rest)

    def get_act(self, name, MT, K):
        return R.unpack_act(self.get(name)[:32 * MT * K], MT, K)

    def put_stats(self, st):
        self.put_front("stats", st.reshape(-1).astype(np.float64), rest=1e300)

    def w(self, key, layer=None):
        return self.sd[key if layer is None else "blocks.%d.%s" % (layer, key)]


_ENGINES = EngineCache()


def _probe(name, kind="dense", env=()):
    key = (name, kind, env)
    live = _ENGINES.engines
    if key not in live and name in ("R3", "R4"):           # the two large shapes: one of them (and its variants) on the device at a time
        for k in [k for k in live if k[0] in ("R3", "R4") and k[0] != name]:
            live.pop(k).close()
        torch.cuda.empty_cache()
    return _ENGINES.get(key, lambda: Probe(name, kind, env))


@pytest.fixture(scope="module", autouse=True)
def engines():
    yield _ENGINES
    _ENGINES.close_all()
    torch.cuda.empty_cache()


def _conds(rs, M, Bhalf=None):
    c = rs.randint(0, NCLS, size=M) + V + 1
    if Bhalf is not None:
        c[Bhalf:] = NONE_ID
    return c.astype(np.int64)


def _warm_caches(pr, rs, upto):
    """random cache rows below `upto` (the same on every engine given the same rs), 3e30 from there on"""
    for l in range(pr.nl):
        for nme in ("kcache", "vcache"):
            c = np.full((pr.Mmax, pr.H, pr.T, pr.hd), GARBAGE, dtype=np.float32)
            c[:, :, :upto] = rs.standard_normal((pr.Mmax, pr.H, upto, pr.hd)).astype(np.float32)
            pr.put(nme, c.reshape(-1), l)


# ------------------------------------------------------------------------------------------------ exact between paths: the walk
WALK = ([("R1", (), M) for M in (1, 5, 31, 32, 33, 63, 64, 65, 127, 128)] + [("R2", (), M) for M in (5, 33, 64, 65, 128)]
        + [("R2", ("WMAR_NO_BX",), M) for M in (65, 128)] + [("R3", (), 33), ("R3", (), 65), ("R4", (), 5), ("R4", (), 65)]
        + [(n, (), M) for n in ("R5", "R6", "R7") for M in (5, 33)])


@pytest.mark.parametrize("name,env,M", WALK, ids=str)
def test_stage_walk_equals_forward_position(name, env, M):
    """positions 0..2 through wmar_rar_forward_position, then position 2 again stage by stage over sentinel-filled work buffers and
    cache rows: the same logits and cache bits (the position is a function of the tokens, the conditions and the cache rows below)"""
    pr = _probe(name, "dense", env)
    pr.plan(M)
    rs = np.random.RandomState(M)
    cond = _conds(rs, M)
    toks = [np.full(M, -1), cond, rs.randint(0, V, size=M)]
    for l in range(pr.nl):
        pr.fill("kcache", GARBAGE, l); pr.fill("vcache", GARBAGE, l)
    for p in range(3):
        lg = pr.forward_position(toks[p], cond, p)
    kv = [(pr.get("kcache", l), pr.get("vcache", l)) for l in range(pr.nl)]
    pr.sentinel_work()
    for l in range(pr.nl):
        for nme, a in zip(("kcache", "vcache"), kv[l]):
            c = a.reshape(pr.Mmax, pr.H, pr.T, pr.hd).copy()
            c[:M, :, 2] = SENT
            pr.put(nme, c.reshape(-1), l)
    lg2 = pr.walk(M, M, 0, 2, tok=toks[2], cond=cond)
    bad = R.diff_bits(lg2, lg)
    cbad = sum(R.diff_bits(pr.get(nme, l).reshape(pr.Mmax, pr.H, pr.T, pr.hd)[:M], a.reshape(pr.Mmax, pr.H, pr.T, pr.hd)[:M])
               for l in range(pr.nl) for nme, a in zip(("kcache", "vcache"), kv[l]))
    other = sum(int(np.count_nonzero(pr.get(nme, l).reshape(pr.Mmax, pr.H, pr.T, pr.hd)[M:] != GARBAGE)) for l in range(pr.nl) for nme in ("kcache", "vcache"))
    _say("walk %s%s M=%d" % (name, "/".join(env), M), logits_bits=bad, cache_bits=cbad, other_rows=other)
    assert np.isfinite(lg).all()
    assert bad == 0 and cbad == 0, "%d logits and %d cache floats differ between the stage walk and forward_position" % (bad, cbad)
    assert other == 0, "%d cache floats of sequences past the batch changed" % other


# ------------------------------------------------------------------------------------------------ exact between paths: shared_u
SHARED = [("R1", B) for B in (1, 5, 31, 32, 33, 63, 64)] + [("R2", B) for B in (5, 33, 64)] + [("R3", B) for B in (31, 33, 64)] + [("R4", B) for B in (5, 33)]


@pytest.mark.parametrize("name,Bhalf", SHARED, ids=str)
def test_shared_u_walk_equals_plain_walk(name, Bhalf):
    """generate's plan (rows >= Bhalf read row p of mod_u, sc / mod have MTc row tiles, the embedding reads ids[m % Bhalf]) against the
    plain plan on the same 2 Bhalf rows.  The shared_u walk finds 3e30 in every table row but p and in every `mod` row at or past
    Bhalf; the plain walk finds the table's row p in its `mod` rows of the unconditional half (and the shared walk's adaLN rows in the
    conditional half: the two adaLN GEMMs differ in shape, the consumers are what is compared)."""
    pr = _probe(name, "dense")
    M, p = 2 * Bhalf, 3
    ps, pp = pr.plan(M, Bhalf, 1), pr.plan(M)
    MT, MTc = ps["MT"], ps["MTc"]
    rs = np.random.RandomState(100 + Bhalf)
    cond = _conds(rs, M, Bhalf)
    ids = rs.randint(0, V, size=(pr.Bmax, pr.SEQ)).astype(np.int64)
    pr.put("ids", ids.reshape(-1))
    # --- the shared_u walk
    pr.sentinel_work()
    _warm_caches(pr, np.random.RandomState(7), p)
    pr.run(R.EMBED, R.ADALN, M, Bhalf, 1, p, cond=cond)                       # builds the table on first use
    table = pr.get("mod_u").reshape(-1, pr.Ntot)
    x_s = pr.get_act("x", MT, pr.D)
    mod_c = R.unpack_act(pr.get("mod")[:32 * MTc * pr.Ntot], MTc, pr.Ntot)
    sc_pad = pr.get("sc")[32 * MTc * pr.D:]
    assert np.all(sc_pad == np.float32(SENT)), "k_rar_embed wrote sc past its %d adaLN row tiles" % MTc
    assert np.all(pr.get("mod")[32 * MTc * pr.Ntot:] == np.float32(SENT)), "the adaLN GEMM wrote mod past its %d row tiles" % MTc
    poisoned = np.full_like(table, GARBAGE)
    poisoned[p] = table[p]
    pr.put("mod_u", poisoned.reshape(-1))
    mod_p = mod_c.copy()
    mod_p[Bhalf:] = GARBAGE
    pr.put_front("mod", R.pack_act(mod_p, MTc), rest=GARBAGE)
    lg_s = pr.walk(M, Bhalf, 1, p, first=R.MOD_IN)
    h_s, xo_s = pr.get_act("h", MT, pr.D), pr.get_act("x", MT, pr.D)
    kv_s = [(pr.get("kcache", l), pr.get("vcache", l)) for l in range(pr.nl)]
    pr.put("mod_u", table.reshape(-1))
    # --- the plain walk on the same rows
    pr.sentinel_work()
    _warm_caches(pr, np.random.RandomState(7), p)
    tok = ids[np.arange(M) % Bhalf, p - 2]
    pr.run(R.EMBED, R.ADALN, M, M, 0, p, tok=tok, cond=cond)
    x_p = pr.get_act("x", MT, pr.D)
    full = np.zeros((32 * MT, pr.Ntot), dtype=np.float32)
    full[:Bhalf] = mod_c[:Bhalf]
    full[Bhalf:M] = table[p][None, :]
    pr.put_front("mod", R.pack_act(full, MT), rest=GARBAGE)
    lg_p = pr.walk(M, M, 0, p, first=R.MOD_IN)
    h_p, xo_p = pr.get_act("h", MT, pr.D), pr.get_act("x", MT, pr.D)
    rows = np.nonzero((lg_s.view(np.uint32) != lg_p.view(np.uint32)).any(1))[0]
    ebad, xbad, hbad = R.diff_bits(x_s[:M], x_p[:M]), R.diff_bits(xo_s[:M], xo_p[:M]), R.diff_bits(h_s[:M], h_p[:M])
    cbad = sum(R.diff_bits(pr.get(nme, l).reshape(pr.Mmax, -1)[:M], a.reshape(pr.Mmax, -1)[:M]) for l in range(pr.nl) for nme, a in zip(("kcache", "vcache"), kv_s[l]))
    _say("shared_u %s Bhalf=%d" % (name, Bhalf), logit_rows=len(rows), embed_bits=ebad, x_bits=xbad, h_bits=hbad, cache_bits=cbad)
    assert np.isfinite(lg_s).all() and np.isfinite(lg_p).all(), "a row read a modulation it must not read (3e30 reached the logits)"
    assert ebad == 0, "the generate form of the embedding (ids[m %% Bhalf]) differs from the explicit tokens in %d floats" % ebad
    assert len(rows) == 0 and xbad == 0 and hbad == 0 and cbad == 0, (
        "shared_u and plain walks differ in rows %s (last conditional row %d, first unconditional row %d, the one behind it %d)" % (
            rows.tolist()[:16], Bhalf - 1, Bhalf, Bhalf + 1))


# ------------------------------------------------------------------------------------------------ exact between paths: fused / pair
FUSED = [("R1", 5), ("R1", 64), ("R1", 128), ("R2", 33), ("R2", 128), ("R3", 65), ("R3", 128), ("R4", 5), ("R4", 65), ("R4", 128)]


def _resid_inputs(pr, plan, M, stage, layer, rs, integer=False):
    """x, slab pieces, packed mod of one RESID_* launch: dense, or integers with power-of-two gates"""
    MT, D = plan["MT"], pr.D
    S = plan["S_proj"] if stage == R.RESID_ATTN else plan["S_fc2"]
    if integer:
        x = rs.randint(-64, 65, size=(32 * MT, D)).astype(np.float32)
        slabs = rs.randint(-512, 513, size=(S, 32 * MT, D)).astype(np.float32)
        mod = (rs.standard_normal((32 * plan["MTc"], pr.Ntot)) * 0.5).astype(np.float32)
        o = R.block_offsets(layer, D)
        g0 = o["gate_msa"] if stage == R.RESID_ATTN else o["gate_mlp"]
        mod[:, g0:g0 + D] = 2.0 ** rs.randint(-2, 3, size=(32 * plan["MTc"], D)) * rs.choice([-1.0, 1.0], size=(32 * plan["MTc"], D))
    else:
        x = rs.standard_normal((32 * MT, D)).astype(np.float32)
        slabs = rs.standard_normal((S, 32 * MT, D)).astype(np.float32)
        mod = (rs.standard_normal((32 * plan["MTc"], pr.Ntot)) * 0.5).astype(np.float32)
    x[M:] = GARBAGE
    return x, slabs, mod


def _load_resid(pr, plan, x, slabs, mod):
    pr.sentinel_work()
    pr.put_act("x", x, plan["MT"])
    buf = np.full(pr.size("slabs") // 4, SENT, dtype=np.float32)
    pr.put("slabs", R.put_pieces(buf, slabs, plan["MT"]))
    pr.put_front("mod", R.pack_act(mod, plan["MTc"]), rest=GARBAGE)
    pr.fill("part", -1)                                             # stale words are poison, never a previous run's sums


def _resid_outputs(pr, plan, stage, layer):
    MT, D = plan["MT"], pr.D
    to_planes = plan["bx"] and stage == R.RESID_MLP and layer + 1 < pr.nl
    site = 2 * layer + (0 if stage == R.RESID_ATTN else 1)
    n = R.site_words(D // 8, MT)
    part = pr.get("part")[site * n:(site + 1) * n].copy()
    return dict(x=pr.get_act("x", MT, D), h=pr.get("xq")[:D // 16 * MT * 3 * 64 * 8].copy() if to_planes else pr.get_act("h", MT, D), part=part, planes=to_planes)


@pytest.mark.parametrize("name,M", FUSED, ids=str)
@pytest.mark.parametrize("stage", [R.RESID_ATTN, R.RESID_MLP], ids=["RESID_ATTN", "RESID_MLP"])
def test_resid_mod_fused_equals_the_two_launch_pair(name, M, stage):
    """k_resid_mod<S, KPW, 0> against <.., 1> + <.., 2> (a WMAR_NO_XR=1 engine of the same weights, the same inputs copied in): the
    same bits of x, h (or the planes) and part"""
    pf, pn = _probe(name, "dense"), _probe(name, "dense", ("WMAR_NO_XR",))
    plan, plan_n = pf.plan(M), pn.plan(M)
    assert plan["fused"] == 1 and plan_n["fused"] == 0
    layer = 0
    x, slabs, mod = _resid_inputs(pf, plan, M, stage, layer, np.random.RandomState(M + stage))
    outs = []
    for pr, pl in ((pf, plan), (pn, plan_n)):
        _load_resid(pr, pl, x, slabs, mod)
        pr.run(stage, stage, M, pos=1, layer=layer)
        outs.append(_resid_outputs(pr, pl, stage, layer))
    a, b = outs
    xb, hb = R.diff_bits(a["x"][:M], b["x"][:M]), (int(np.count_nonzero(a["h"] != b["h"])) if a["planes"] else R.diff_bits(a["h"][:M], b["h"][:M]))
    Mpad = 32 * plan["MT"]
    pa, pb = a["part"].reshape(-1, Mpad, 2)[:, :M], b["part"].reshape(-1, Mpad, 2)[:, :M]
    pbad = int(np.count_nonzero(pa != pb))
    _say("fused/pair %s M=%d %s" % (name, M, R.STAGES[stage]), x_bits=xb, h_bits=hb, part_bits=pbad, kernel=plan["roles"]["resid_attn" if stage == R.RESID_ATTN else "resid_mlp"])
    assert not np.any(pa == R.POISON), "a live partial sum is still poison"
    assert xb == 0 and hb == 0 and pbad == 0, "fused and two-launch k_resid_mod differ: x %d, h %d, part %d" % (xb, hb, pbad)


# ------------------------------------------------------------------------------------------------ held to float64: RESID_* and MOD_IN
RESID = [("R1", 1, 0), ("R1", 31, 0), ("R1", 32, 0), ("R1", 63, 0), ("R1", 127, 0), ("R1", 62, 31), ("R1", 126, 63), ("R1", 5, 0), ("R1", 33, 0), ("R1", 128, 0), ("R1", 66, 33), ("R1", 64, 32), ("R2", 128, 0), ("R2", 66, 33), ("R3", 128, 64), ("R3", 65, 0),
         ("R4", 5, 0), ("R4", 65, 0), ("R4", 128, 0), ("R4", 66, 33)]


@pytest.mark.parametrize("name,M,Bhalf", RESID, ids=str)
@pytest.mark.parametrize("stage", [R.RESID_ATTN, R.RESID_MLP], ids=["RESID_ATTN", "RESID_MLP"])
@pytest.mark.parametrize("integer", [True, False], ids=["int", "dense"])
def test_resid_mod_against_float64(name, M, Bhalf, stage, integer):
    """one k_resid_mod launch: x' (exact on integer operands with power-of-two gates, else within the fold's derived distance), the
    published partial sums, every buffer it does not own, and h / the planes per element to the normaliser rule.  Bhalf > 0: shared_u,
    rows at or past Bhalf take gate / shift / scale from row p of the table, which holds 3e30 everywhere else."""
    pr = _probe(name, "int" if integer else "dense")       # integer: integer biases too, so x' is a multiple of 1/4 below 2^14
    shared = 1 if Bhalf else 0
    plan = pr.plan(M, Bhalf or M, shared)
    MT, MTc, D, KB = plan["MT"], plan["MTc"], pr.D, pr.D // 8
    layer, p = 0, 5
    rs = np.random.RandomState(31 * M + stage + (1 if integer else 0))
    x, slabs, mod = _resid_inputs(pr, plan, M, stage, layer, rs, integer)
    if shared:
        pr.run(R.EMBED, R.EMBED, M, Bhalf, 1, p, cond=_conds(rs, M, Bhalf))      # (builds the table once; its contents are replaced)
        table = np.full((pr.size("mod_u") // 4 // pr.Ntot, pr.Ntot), GARBAGE, dtype=np.float32)
        row = (rs.standard_normal(pr.Ntot) * 0.5).astype(np.float32)
        if integer:
            o = R.block_offsets(layer, D)
            for g0 in (o["gate_msa"], o["gate_mlp"]):
                row[g0:g0 + D] = 2.0 ** rs.randint(-2, 3, size=D)
        table[p] = row
        mod[Bhalf:] = GARBAGE
    _load_resid(pr, plan, x, slabs, mod)
    if shared:
        keep = pr.get("mod_u")
        pr.put("mod_u", table.reshape(-1))
    snap = pr.snapshot()
    pr.run(stage, stage, M, Bhalf or M, shared, pos=p, layer=layer)
    out = _resid_outputs(pr, plan, stage, layer)
    site, nw = 2 * layer + (0 if stage == R.RESID_ATTN else 1), R.site_words(KB, MT)
    pr.assert_unowned_unchanged(snap, {"x", "xq" if out["planes"] else "h"}, (site * nw, (site + 1) * nw))
    if shared:
        pr.put("mod_u", keep)
    eff = R.effective_mod(mod, table if shared else None, p, M, Bhalf, shared)
    o = R.block_offsets(layer, D)
    last = layer + 1 == pr.nl
    if stage == R.RESID_ATTN:
        g0, sh0, sc0, bias = o["gate_msa"], o["shift_mlp"], o["scale_mlp"], pr.w("attn.proj.bias", layer)
        gamma, beta = pr.w("norm2.weight", layer), pr.w("norm2.bias", layer)
    else:
        g0, bias = o["gate_mlp"], pr.w("mlp.fc2.bias", layer)
        if last:
            fo = R.final_offsets(pr.nl, D)
            sh0, sc0, gamma, beta = fo["shift"], fo["scale"], None, None
        else:
            o2 = R.block_offsets(layer + 1, D)
            sh0, sc0, gamma, beta = o2["shift_msa"], o2["scale_msa"], pr.w("norm1.weight", layer + 1), pr.w("norm1.bias", layer + 1)
    gate = eff[:, g0:g0 + D]
    xg = out["x"]
    if integer:
        xbad = R.diff_bits(xg[:M], R.gated_fold32(x[:M], gate, bias, [s[:M] for s in slabs]))
        assert xbad == 0, "gated fold: %d of %d fp32 patterns differ on integer operands" % (xbad, M * D)
        xr = 0.0
    else:
        v, tol = R.gated_fold64(x[:M], gate, bias, [s[:M] for s in slabs])
        xr = float((np.abs(xg[:M].astype(np.float64) - v) / tol).max())
        assert xr <= 1.0, "gated fold: worst element %.3g x the derived distance" % xr
    chunks = R.rm_chunk_lists(KB)
    part = out["part"].view(np.float64).reshape(len(chunks), 32 * MT, 2)
    assert not np.any(out["part"].reshape(len(chunks), 32 * MT, 2)[:, :M] == R.POISON)
    sw = R.check_stats(part, xg, chunks, M, exact=integer)
    sums = R.rm_row_sums(part[:, :M])
    if out["planes"]:
        hval = R.check_planes_consistent(out["h"], MT, D, M, "xq planes")
    else:
        hval = out["h"]
    hr, yr = R.check_modulate(hval, xg, sums, D, gamma, beta, eff[:, sc0:sc0 + D], eff[:, sh0:sh0 + D], M, R.STAGES[stage])
    _say("resid %s M=%d Bhalf=%d %s %s" % (name, M, Bhalf, R.STAGES[stage], "int" if integer else "dense"), fold=xr, stats=sw, h=hr, h_fp32=yr,
         kpw=plan["kpw"], nrm=plan["nrm"], planes=int(out["planes"]))


MODIN = [("R1", 1, 0), ("R1", 31, 0), ("R1", 32, 0), ("R1", 63, 0), ("R1", 127, 0), ("R1", 62, 31), ("R1", 126, 63), ("R1", 5, 0), ("R1", 128, 0), ("R1", 66, 33), ("R2", 128, 0), ("R3", 128, 64), ("R4", 5, 0), ("R4", 65, 0), ("R4", 66, 33), ("R4", 128, 0)]


@pytest.mark.parametrize("name,M,Bhalf", MODIN, ids=str)
def test_modulate_against_float64(name, M, Bhalf):
    """k_modulate (MOD_IN): statistics of 1 .. 17 chunks (R4: the second round of the 16-wide loop), own rows from the packed mod with
    MTc row tiles, shared rows from row p of the table; h or the xq planes per element to the normaliser rule"""
    pr = _probe(name, "dense")
    shared = 1 if Bhalf else 0
    plan = pr.plan(M, Bhalf or M, shared)
    MT, MTc, D, KB, p = plan["MT"], plan["MTc"], pr.D, pr.D // 8, 4
    rs = np.random.RandomState(17 * M + Bhalf)
    x = (rs.standard_normal((32 * MT, D)) + rs.standard_normal((32 * MT, 1))).astype(np.float32)
    mod = (rs.standard_normal((32 * MTc, pr.Ntot)) * 0.5).astype(np.float32)
    chunks = R.stat_chunk_lists(KB)
    assert len(chunks) == plan["nch"]
    st = R.stats_ref(x, chunks)
    table = None
    if shared:
        pr.run(R.EMBED, R.EMBED, M, Bhalf, 1, p, cond=_conds(rs, M, Bhalf))
        table = np.full((pr.size("mod_u") // 4 // pr.Ntot, pr.Ntot), GARBAGE, dtype=np.float32)
        table[p] = (rs.standard_normal(pr.Ntot) * 0.5).astype(np.float32)
        mod[Bhalf:] = GARBAGE
        keep = pr.get("mod_u")
        pr.put("mod_u", table.reshape(-1))
    pr.sentinel_work()
    pr.put_act("x", x, MT)
    pr.put_stats(st)
    pr.put_front("mod", R.pack_act(mod, MTc), rest=GARBAGE)
    snap = pr.snapshot()
    pr.run(R.MOD_IN, R.MOD_IN, M, Bhalf or M, shared, pos=p)
    pr.assert_unowned_unchanged(snap, {"xq" if plan["bx"] else "h"})
    if shared:
        pr.put("mod_u", keep)
    eff = R.effective_mod(mod, table, p, M, Bhalf, shared)
    o = R.block_offsets(0, D)
    if plan["bx"]:
        hval = R.check_planes_consistent(pr.get("xq")[:D // 16 * MT * 3 * 64 * 8], MT, D, M, "xq planes")
        assert np.all(pr.get("h") == np.float32(SENT)), "h written on the bx plan"
    else:
        hval = pr.get_act("h", MT, D)
    hr, yr = R.check_modulate(hval, x, R.mod_row_sums(st[:, :M]), D, pr.w("norm1.weight", 0), pr.w("norm1.bias", 0), eff[:, o["scale_msa"]:o["scale_msa"] + D],
                              eff[:, o["shift_msa"]:o["shift_msa"] + D], M, "MOD_IN")
    assert R.diff_bits(pr.get_act("x", MT, D), x) == 0, "x changed"
    _say("mod_in %s M=%d Bhalf=%d" % (name, M, Bhalf), h=hr, h_fp32=yr, nch=plan["nch"], planes=plan["bx"])


# ------------------------------------------------------------------------------------------------ the embedding
EMB = [("R1", 1, 0), ("R1", 31, 0), ("R1", 32, 0), ("R1", 63, 0), ("R1", 127, 0), ("R1", 62, 31), ("R1", 126, 63), ("R1", 5, 0), ("R1", 128, 0), ("R1", 66, 33), ("R1", 2, 1), ("R2", 64, 32), ("R3", 66, 33), ("R3", 128, 64), ("R4", 65, 0), ("R4", 66, 33)]


@pytest.mark.parametrize("name,M,Bhalf", EMB, ids=str)
@pytest.mark.parametrize("p", [0, 1, 2, 9])
@pytest.mark.parametrize("kind", ["int", "dense"])
def test_embedding_both_forms(name, M, Bhalf, p, kind):
    """k_rar_embed: x exact (three fp32 additions in a fixed order) in forward_position's form with explicit tokens where Bhalf is 0
    and generate's three cases otherwise; its fp64 statistics exact on integer embeddings and within K 2^-53 of their scale on dense
    ones; SiLU(c) within 7 x 2^-24 of the float64 value, its planes the split of the same fp32 values,
    nothing written past the adaLN row tiles"""
    pr = _probe(name, kind)
    shared = 1 if Bhalf else 0
    plan = pr.plan(M, Bhalf or M, shared)
    MT, MTc, D, KB = plan["MT"], plan["MTc"], pr.D, pr.D // 8
    rs = np.random.RandomState(1000 * p + M)
    cond = _conds(rs, M, Bhalf or None)
    ids = rs.randint(0, V, size=(pr.Bmax, pr.SEQ)).astype(np.int64)
    pr.put("ids", ids.reshape(-1))
    tok = None if shared else np.where(rs.rand(M) < 0.2, -1, rs.randint(0, V, size=M))
    pr.sentinel_work()
    pr.run(R.EMBED, R.EMBED, M, Bhalf or M, shared, p, tok=tok, cond=cond)
    tk = R.embed_tokens(tok, cond, ids, pr.SEQ, Bhalf or M, p, M)
    want = R.embed_x(pr.w("embeddings.weight"), pr.w("cls_token")[0, 0], pr.w("pos_embed")[0], pr.w("target_aware_pos_embed")[0], tk, p)
    xg = pr.get_act("x", MT, D)
    R.check_exact(xg[:M], want, "embedding x")
    chunks = R.stat_chunk_lists(KB)
    sw = R.check_stats(pr.get("stats")[:len(chunks) * 32 * MT * 2].reshape(len(chunks), 32 * MT, 2), xg, chunks, M, exact=kind == "int")
    n_sc = min(M, 32 * MTc)
    c = R.cond_c(pr.w("embeddings.weight"), pr.w("timesteps_embeddings")[0], cond[:n_sc], p)
    scg = R.unpack_act(pr.get("sc")[:32 * MTc * D], MTc, D)
    sr, s32 = R.check_silu(scg[:n_sc], c)
    assert np.all(pr.get("sc")[32 * MTc * D:] == np.float32(SENT)), "sc written past its %d row tiles" % MTc
    if plan["ada_bx"]:
        R.check_planes(pr.get("scq")[:D // 16 * MTc * 3 * 64 * 8], scg, MTc, D, n_sc, "scq planes")
    elif pr.has("scq"):
        assert np.all(pr.get("scq") == 0x7f7f), "scq written off the k_bx adaLN plan"
    for nme in ("h", "y", "mod", "hbuf"):
        assert np.all(pr.get(nme) == np.float32(SENT)), "%s changed" % nme
    _say("embed %s %s M=%d Bhalf=%d p=%d" % (name, kind, M, Bhalf, p), x_bits=0, stats=sw, silu=sr, silu_fp32=s32, MTc=MTc, planes=plan["ada_bx"])


# ------------------------------------------------------------------------------------------------ the unconditional table
@pytest.mark.parametrize("name", ["R1", "R2", "R4"])
def test_unconditional_table(name):
    """k_rar_cond_rows + the table GEMM: every row p < T of mod_u within DENSE_GATE = 2 x the sequential fp32 chain of SiLU(emb[none] + timesteps[p])
    Wada^T + bada (normalised by sum |terms|), the SiLU's own derived distance carried through the magnitudes"""
    pr = _probe(name, "dense")
    pr.run(R.EMBED, R.EMBED, 2, 1, 1, 0, cond=np.array([V + 1, NONE_ID]))
    tab = pr.get("mod_u").reshape(-1, pr.Ntot)[:pr.T]
    ref, mag, c = R.uncond_table64(pr.w("embeddings.weight"), pr.w("timesteps_embeddings")[0], NONE_ID, pr.T, pr.wada, pr.bada)
    s32 = R.silu32(c)
    chain = R.gemm_chain(pr.wada, s32, R.uniform_ranges(pr.Ntot // 32, lambda s: (0, pr.D // 8), 1))[0] + pr.bada[None, :]
    e = float((np.abs(tab.astype(np.float64) - ref) / mag).max())
    ec = float((np.abs(chain.astype(np.float64) - ref) / mag).max())
    _say("table %s" % name, err=e, chain=ec, ratio=e / ec)
    assert e <= R.DENSE_GATE * ec + R.SILU_REL, "table: normalised error %.3g against the chain's %.3g" % (e, ec)


# ------------------------------------------------------------------------------------------------ attention, mode 1
ATT = [("R1", 1), ("R1", 31), ("R1", 32), ("R1", 63), ("R1", 127), ("R1", 5), ("R2", 33), ("R2", 65), ("R3", 65), ("R4", 5), ("R4", 65), ("R5", 5), ("R6", 33), ("R7", 5)]


def _att_lengths(hd, T):
    E = 8 if hd == 80 else R.attn_chunk_rows(hd)
    return E, sorted({t for t in (1, E - 1, E, E + 1, 2 * E + 1, T) if 1 <= t <= T})


def _att_launch(pr, plan, M, Tn, mode):
    """one ATTN launch at Tn cached rows (the new one included) on random pieces and caches; returns everything the checks need"""
    MT, D, H, hd, S, rm = plan["MT"], pr.D, pr.H, pr.hd, plan["S_qkv"], bool(plan["rowmajor"])
    scale = 1.0 / np.sqrt(hd)
    rs = np.random.RandomState(Tn * 131 + M)
    P = (rs.standard_normal((S, 32 * MT, 3 * D)) * (0.7 / np.sqrt(S))).astype(np.float32)
    P[:, M:] = GARBAGE
    kc = rs.standard_normal((pr.Mmax, H, pr.T, hd)).astype(np.float32)
    vc = rs.standard_normal((pr.Mmax, H, pr.T, hd)).astype(np.float32)
    pro = R.attn_prologue(P[:, :M], pr.w("attn.qkv.bias", 0), pr.w("attn.q_norm.weight", 0), pr.w("attn.q_norm.bias", 0),
                          pr.w("attn.k_norm.weight", 0), pr.w("attn.k_norm.bias", 0), H, hd)
    q32 = pro[1][0]
    win = None
    if mode == "onehot" and Tn > 1:
        # every (row, head) has ONE cached row aligned with its q, far ahead of the others and of the new row: the output is that V row
        win = rs.randint(0, Tn - 1, size=(M, H))
        kc[:, :, :Tn - 1] *= 0.01
        n2 = np.maximum((q32.astype(np.float64) ** 2).sum(-1, keepdims=True), 1e-12)
        kc[np.arange(M)[:, None], np.arange(H)[None, :], win] = (q32 * (400.0 / scale) / n2).astype(np.float32)
    kc[:, :, Tn - 1:] = GARBAGE
    vc[:, :, Tn - 1:] = GARBAGE
    pr.sentinel_work()
    buf = np.full(pr.size("qkv_slabs") // 4, SENT, dtype=np.float32)
    pr.put("qkv_slabs", R.put_pieces(buf, P, MT, rm))
    pr.put("kcache", kc.reshape(-1)); pr.put("vcache", vc.reshape(-1))
    snap = pr.snapshot()
    pr.run(R.ATTN, R.ATTN, M, pos=Tn - 1, layer=0)
    pr.assert_unowned_unchanged(snap, {"yq" if plan["bx"] else "y"})
    return pro, kc, vc, pr.get("kcache").reshape(kc.shape), pr.get("vcache").reshape(vc.shape), win


@pytest.mark.parametrize("name,M", ATT, ids=str)
@pytest.mark.parametrize("mode", ["onehot", "dense"])
def test_attention_mode1(name, M, mode):
    """k_attn_decode<HD,1,1> / k_attn_decode80<1> (packed and row-major pieces) at every chunk edge of the cache: the appended k-normed
    row per element within the distance derived from the prologue's operation count, the plain v row bit for bit, cache rows below the
    position and other rows' caches untouched, and the output -- one-hot: exactly the selected V row (one cached row: the new V row);
    dense: the derived distance per output and 4 x an fp32 numpy evaluation per launch"""
    pr = _probe(name, "dense")
    plan = pr.plan(M)
    MT, D, H, hd, S, rm = plan["MT"], pr.D, pr.H, pr.hd, plan["S_qkv"], bool(plan["rowmajor"])
    assert ("k_attn_decode80<1>" if hd == 80 else "k_attn_decode<%d,1,1>" % hd) in plan["roles"]["attn"]
    E, lengths = _att_lengths(hd, pr.T)
    scale = 1.0 / np.sqrt(hd)
    figs = dict(kdist=0.0, dist=0.0, fp32=0.0)
    late = []                                                    # appended-row misses: raised behind the loop, so that every length is still run
    for Tn in lengths:
        ((q64, k64, v64), (q32, k32, v32), (nq, nk_, nv_)), kc, vc, kg, vg, win = _att_launch(pr, plan, M, Tn, mode)
        R.check_cache_untouched(kg, kc, M, Tn - 1, H, pr.T, hd)
        R.check_cache_untouched(vg, vc, M, Tn - 1, H, pr.T, hd)
        kerr = np.abs(kg[:M, :, Tn - 1].astype(np.float64) - k64) / R.prologue_tol(nk_, hd)
        if not np.all(kerr <= 1.0):
            k32err = np.abs(k32.astype(np.float64) - k64) / R.prologue_tol(nk_, hd)
            late.append("%d rows: worst element %.3g x the derived distance (the fp32 numpy evaluation in the prologue's order: %.3g x)" % (
                Tn, float(kerr.max()), float(k32err.max())))
        figs["kdist"] = max(figs["kdist"], float(kerr.max()))
        R.check_exact(vg[:M, :, Tn - 1], v32, "appended V row")          # pieces in the prologue's order + bias: the bits are fixed
        if plan["bx"]:
            y = R.check_planes_consistent(pr.get("yq")[:D // 16 * MT * 3 * 64 * 8], MT, D, M, "yq planes")[:M].reshape(M, H, hd)
            assert np.all(pr.get("y") == np.float32(SENT)), "y written on the bx plan"
        else:
            y = pr.get_act("y", MT, D)[:M].reshape(M, H, hd)
        K64 = np.concatenate([kc[:M, :, :Tn - 1].astype(np.float64), kg[:M, :, Tn - 1:Tn].astype(np.float64)], 2)
        V64 = np.concatenate([vc[:M, :, :Tn - 1].astype(np.float64), vg[:M, :, Tn - 1:Tn].astype(np.float64)], 2)
        if mode == "onehot" and Tn == 1:
            R.check_onehot(y, vg[:M, :, 0], "new-token attention")
        elif mode == "onehot":
            R.check_onehot(y, vc[np.arange(M)[:, None], np.arange(H)[None, :], win])
        else:
            # the cache's new row is what the kernel itself wrote (held above); q is held through the bound's dq
            ref, tol = R.attn_dense_bound(q64, R.prologue_tol(nq, hd), K64, np.zeros_like(q64), V64, np.zeros_like(q64), scale, E, 1)
            figs["dist"] = max(figs["dist"], R.check_attn_dense(y, ref, tol))
            y32 = R.attn_fp32(q32, K64, V64, scale)
            e, e32 = float(np.abs(y - ref).max()), float(np.abs(y32 - ref).max())
            assert e <= 4.0 * e32, "attention at %d rows: largest error %.3g against the fp32 evaluation's %.3g (gate 4 x)" % (Tn, e, e32)
            if e32 > 0:
                figs["fp32"] = max(figs["fp32"], e / e32)
    _say("attn %s M=%d %s" % (name, M, mode), lengths=len(lengths), appended_of_distance=figs["kdist"], of_distance=figs["dist"], x_fp32=figs["fp32"],
         rowmajor=int(rm), S=S)
    assert not late, "appended K row at " + "; ".join(late)


@pytest.mark.parametrize("name,M", ATT, ids=str)
def test_appended_rows_within_twice_the_fp32_algebra(name, M):
    """The appended k-normed row of every ATTN launch: largest normalised error within 2 x that of an fp32 numpy evaluation of the
    prologue's own algebra in the prologue's own summation order (rar_kernel_reference.attn_prologue: the pieces per row group, then
    the groups; four values per lane, then the lanes' butterfly).  Measured 1.00 .. 1.25 x.  (Against an evaluation that adds in
    numpy's pairwise order instead, the same kernels measured up to 2.20 x: the order belongs to the algebra.)"""
    pr = _probe(name, "dense")
    plan = pr.plan(M)
    hd = pr.hd
    late, worst = [], 0.0
    for Tn in _att_lengths(hd, pr.T)[1]:
        ((q64, k64, v64), (q32, k32, v32), (nq, nk_, nv_)), kc, vc, kg, vg, win = _att_launch(pr, plan, M, Tn, "dense")
        kn, kref = np.maximum(nk_.reshape(M, -1), 1e-300), k64.reshape(M, -1)
        e_k = float((np.abs(kg[:M, :, Tn - 1].reshape(M, -1).astype(np.float64) - kref) / kn).max())
        e_y = float((np.abs(k32.reshape(M, -1).astype(np.float64) - kref) / kn).max())
        worst = max(worst, e_k / e_y)
        if e_k > 2.0 * e_y:
            late.append("%d cached rows: normalised error %.3g is %.2f x the fp32 algebra's %.3g" % (Tn, e_k, e_k / e_y, e_y))
    _say("appended %s M=%d" % (name, M), x_fp32=worst)
    assert not late, "appended K row at " + "; ".join(late)


# ------------------------------------------------------------------------------------------------ packed weights, integer GEMM stages
@pytest.mark.parametrize("name", ["R1", "R2", "R3", "R4", "R5"])
def test_packed_weights_both_orders(name):
    """k_pack_linear and k_pack_bx: every packed weight of the engine bit for bit, the adaLN matrix as ONE matrix of Ntot rows"""
    pr = _probe(name, "dense")
    n = 0
    for l in range(pr.nl):
        for buf, key in (("wqkv", "attn.qkv.weight"), ("wproj", "attn.proj.weight"), ("wfc1", "mlp.fc1.weight"), ("wfc2", "mlp.fc2.weight")):
            R.check_pack(pr.get(buf, l), R.pack_linear(pr.w(key, l)), buf)
            n += 1
            if pr.has(buf + "_bx"):
                R.check_pack(pr.get(buf + "_bx", l), R.pack_bx(pr.w(key, l)), buf + "_bx")
                n += 1
    R.check_pack(pr.get("wada"), R.pack_linear(pr.wada), "wada")
    R.check_pack(pr.get("whead"), R.pack_linear(pr.w("lm_head.weight")), "whead")
    R.check_pack(pr.get("bada"), pr.bada, "bada")
    if pr.has("wada_bx"):
        R.check_pack(pr.get("wada_bx"), R.pack_bx(pr.wada), "wada_bx")
        n += 1
    assert pr.has("wqkv_bx") == (name in ("R2", "R3")) and pr.has("wfc1_bx") == (name == "R3") and pr.has("wada_bx") == (name == "R3")
    _say("packs %s" % name, packs=n + 3, differing_bits=0)


GEMMS = [("R1", (), 1, 0), ("R1", (), 31, 0), ("R1", (), 32, 0), ("R1", (), 63, 0), ("R1", (), 127, 0), ("R1", (), 5, 0), ("R1", (), 64, 0), ("R1", (), 128, 0), ("R2", (), 33, 0), ("R2", (), 128, 0), ("R2", ("WMAR_NO_BX",), 128, 0),
         ("R3", (), 64, 0), ("R3", (), 128, 64), ("R3", (), 65, 0), ("R4", (), 5, 0), ("R4", (), 65, 0)]


def _quarters(rs, Mpad, K, M):
    """sparse multiples of 1/4: exact in fp32 and in the first bf16 piece, pre-activations of a few units"""
    X = (rs.randint(-2, 3, size=(Mpad, K)) * 0.25 * (rs.rand(Mpad, K) < 1.0 / 16)).astype(np.float32)
    X[M:] = GARBAGE
    return X


@pytest.mark.parametrize("name,env,M,Bhalf", GEMMS, ids=str)
def test_gemm_stages_on_integer_operands(name, env, M, Bhalf):
    """ADALN, QKV, PROJ, FC2 and HEAD on integer weights: every piece equals the partial sum over exactly its k-blocks bit for bit (the
    packed and the row-major form, k_gemm and k_bx at the plan's PER / S), pieces past the plan keep the sentinel; FC1's GELU (k_gemm
    and the XF k_bx) within the derived distance of gelu(exact pre-activation), its planes the split of those values"""
    pr = _probe(name, "int", env)
    shared = 1 if Bhalf else 0
    plan = pr.plan(M, Bhalf or M, shared)
    MT, MTc, D, F, KB, bx = plan["MT"], plan["MTc"], pr.D, pr.F, pr.D // 8, plan["bx"]
    rs = np.random.RandomState(M + D)
    figs = {}
    if shared:
        pr.run(R.EMBED, R.EMBED, M, Bhalf, 1, 0, cond=_conds(rs, M, Bhalf))

    def slabs_of(bufname, N, P, rowmajor=False):
        return R.get_pieces(pr.get(bufname), P, MT, N, rowmajor)

    def load_in(fp32_name, planes_name, X, planes, MTx=MT):
        pr.sentinel_work()
        for nme in ("slabs", "qkv_slabs"):
            pr.fill(nme, SENT)
        if planes:
            pr.put_front(planes_name, R.pack_planes(X, MTx))
        else:
            pr.put_act(fp32_name, X, MTx)

    # ADALN: sc (or its planes) -> packed mod with MTc row tiles
    n_c = min(M, 32 * MTc) if not shared else Bhalf
    X = _quarters(rs, 32 * MTc, D, n_c)
    load_in("sc", "scq", X, plan["ada_bx"], MTc)
    pr.run(R.ADALN, R.ADALN, M, Bhalf or M, shared, 1)
    modg = R.unpack_act(pr.get("mod")[:32 * MTc * pr.Ntot], MTc, pr.Ntot)
    want = (X[:n_c].astype(np.float64) @ pr.wada.astype(np.float64).T + pr.bada.astype(np.float64)[None, :]).astype(np.float32)
    R.check_exact(modg[:n_c], want, "adaLN GEMM (%s)" % plan["roles"]["adaln"])
    assert np.all(pr.get("mod")[32 * MTc * pr.Ntot:] == np.float32(SENT)), "mod written past its %d row tiles" % MTc
    # QKV
    X = _quarters(rs, 32 * MT, D, M)
    load_in("h", "xq", X, bx)
    pr.run(R.QKV, R.QKV, M, Bhalf or M, shared, 1, 0)
    S = plan["S_qkv"]
    rng = R.bx_ranges(3 * D // 32, S, plan["PER_qkv"]) if bx else R.gemm_ranges(KB, 3 * D // 32, S)
    R.check_gemm_exact(slabs_of("qkv_slabs", 3 * D, S, bool(plan["rowmajor"])), pr.w("attn.qkv.weight", 0), X, rng, M)
    # PROJ
    X = _quarters(rs, 32 * MT, D, M)
    load_in("y", "yq", X, bx)
    pr.run(R.PROJ, R.PROJ, M, Bhalf or M, shared, 1, 0)
    S = plan["S_proj"]
    rng = R.bx_ranges(D // 32, S, plan["PER_proj"]) if bx else R.gemm_ranges(KB, D // 32, S)
    R.check_gemm_exact(slabs_of("slabs", D, min(S + 1, 8)), pr.w("attn.proj.weight", 0), X, rng, M)
    # FC2
    X = _quarters(rs, 32 * MT, F, M)
    load_in("hbuf", "hq", X, bx)
    pr.run(R.FC2, R.FC2, M, Bhalf or M, shared, 1, 0)
    S = plan["S_fc2"]
    rng = R.bx_ranges(D // 32, S, plan["PER_fc2"]) if bx else R.gemm_ranges(F // 8, D // 32, S)
    R.check_gemm_exact(slabs_of("slabs", D, min(S + 1, 8)), pr.w("mlp.fc2.weight", 0), X, rng, M)
    # FC1 + GELU
    X = _quarters(rs, 32 * MT, D, M)
    load_in("h", None, X, False)
    pr.run(R.FC1, R.FC1, M, Bhalf or M, shared, 1, 0)
    pre = (X[:M].astype(np.float64) @ pr.w("mlp.fc1.weight", 0).astype(np.float64).T + pr.w("mlp.fc1.bias", 0).astype(np.float64)[None, :]).astype(np.float32)
    if bx:                       # the activation goes out as bf16 pieces INSTEAD of fp32 rows (k_gemm<EPI_GELU> with planes, or the XF k_bx)
        val = R.check_planes_consistent(pr.get("hq")[:F // 16 * MT * 3 * 64 * 8], MT, F, M, "hq planes")
        assert np.all(pr.get("hbuf") == np.float32(SENT)), "hbuf written on the bx plan"
    else:
        val = pr.get_act("hbuf", MT, F)
    figs["gelu"] = R.check_gelu(val[:M], pre, "FC1 (%s)" % plan["roles"]["fc1"])
    # HEAD
    X = _quarters(rs, 32 * MT, D, M)
    load_in("h", None, X, False)
    lg = pr.run(R.HEAD, R.HEAD, M, Bhalf or M, shared, 1, pr.nl - 1, want_logits=True)
    want = (X[:M].astype(np.float64) @ pr.w("lm_head.weight").astype(np.float64).T + pr.w("lm_head.bias").astype(np.float64)[None, :]).astype(np.float32)
    R.check_exact(lg, want, "head")
    _say("gemms %s%s M=%d Bhalf=%d" % (name, "/".join(env), M, Bhalf), pieces_bits=0, gelu=figs["gelu"], bx=bx, S="%d/%d/%d" % (plan["S_qkv"], plan["S_proj"], plan["S_fc2"]),
         PER="%d/%d/%d" % (plan["PER_qkv"], plan["PER_proj"], plan["PER_fc2"]), adaln=plan["roles"]["adaln"], fc1=plan["roles"]["fc1"])


DENSE = [("R1", (), 1), ("R1", (), 31), ("R1", (), 63), ("R1", (), 127), ("R3", (), 64), ("R3", (), 128), ("R1", (), 5), ("R1", (), 128), ("R2", (), 33), ("R2", (), 128), ("R3", (), 65), ("R4", (), 5), ("R4", (), 65)]


@pytest.mark.parametrize("name,env,M", DENSE, ids=str)
def test_gemm_pieces_and_head_dense(name, env, M):
    """QKV, PROJ and FC2 pieces, the adaLN GEMM and the head on full-significand operands: per piece, max |got - exact| / sum |terms|
    within DENSE_GATE x the same figure of the sequential fp32 chain over the piece's own k-blocks (the chain bound of the Taming file).
    Full significands need all three bf16 pieces of the k_bx operands (the weights split in registers, the scq / xq / yq / hq planes,
    the XF activation): a dropped or swapped piece is 2^-16 of a term against a chain error of 2^-22.  FC1: gelu of the float64
    pre-activation within the GELU distance, the pre-activation itself allowed DENSE_GATE x the chain's normalised error."""
    pr = _probe(name, "dense", env)
    plan = pr.plan(M)
    MT, D, F, KB, bx = plan["MT"], pr.D, pr.F, pr.D // 8, plan["bx"]
    rs = np.random.RandomState(3 * M + D)
    figs = {}
    for stage, wkey, src, planes, K, N, S, PER, dst in ((R.QKV, "attn.qkv.weight", "h", "xq", D, 3 * D, plan["S_qkv"], plan["PER_qkv"], "qkv_slabs"),
                                                        (R.PROJ, "attn.proj.weight", "y", "yq", D, D, plan["S_proj"], plan["PER_proj"], "slabs"),
                                                        (R.FC2, "mlp.fc2.weight", "hbuf", "hq", F, D, plan["S_fc2"], plan["PER_fc2"], "slabs")):
        X = rs.standard_normal((32 * MT, K)).astype(np.float32)
        X[M:] = GARBAGE
        pr.sentinel_work()
        if bx:
            pr.put_front(planes, R.pack_planes(X, MT))
        else:
            pr.put_act(src, X, MT)
        pr.run(stage, stage, M, pos=1, layer=0)
        rng = R.bx_ranges(N // 32, S, PER) if bx else R.gemm_ranges(K // 8, N // 32, S)
        got = R.get_pieces(pr.get(dst), S, MT, N, bool(plan["rowmajor"]) and stage == R.QKV)
        figs[R.STAGES[stage]] = R.check_gemm_dense(got, pr.w(wkey, 0), X, rng, M)[2]
    # ADALN on dense SiLU rows (k_gemm, or k_bx<4,20,2> with its in-register weight split and all three scq planes)
    MTc = plan["MTc"]
    n_c = min(M, 32 * MTc)
    X = rs.standard_normal((32 * MTc, D)).astype(np.float32)
    X[n_c:] = GARBAGE
    pr.sentinel_work()
    if plan["ada_bx"]:
        pr.put_front("scq", R.pack_planes(X, MTc))
    else:
        pr.put_act("sc", X, MTc)
    pr.run(R.ADALN, R.ADALN, M, pos=1)
    modg = R.unpack_act(pr.get("mod")[:32 * MTc * pr.Ntot], MTc, pr.Ntot)[:n_c]
    ref = X[:n_c].astype(np.float64) @ pr.wada.astype(np.float64).T + pr.bada.astype(np.float64)[None, :]
    mag = np.abs(X[:n_c].astype(np.float64)) @ np.abs(pr.wada.astype(np.float64)).T + np.abs(pr.bada.astype(np.float64))[None, :]
    chain = (R.gemm_chain(pr.wada, X[:n_c], R.uniform_ranges(pr.Ntot // 32, lambda s: (0, KB), 1))[0] + pr.bada[None, :]).astype(np.float32)
    e, ec = float((np.abs(modg - ref) / mag).max()), float((np.abs(chain - ref) / mag).max())
    assert e <= R.DENSE_GATE * ec, "adaLN GEMM (%s): normalised error %.3g is %.2f x the fp32 chain's %.3g" % (plan["roles"]["adaln"], e, e / ec, ec)
    figs["ADALN"] = e / ec
    # FC1 on dense rows: gelu(pre-activation), the pre-activation allowed DENSE_GATE x the chain's normalised error of its own magnitude
    X = rs.standard_normal((32 * MT, D)).astype(np.float32)
    X[M:] = GARBAGE
    pr.sentinel_work()
    pr.put_act("h", X, MT)
    pr.run(R.FC1, R.FC1, M, pos=1, layer=0)
    W1, b1 = pr.w("mlp.fc1.weight", 0), pr.w("mlp.fc1.bias", 0)
    pre = X[:M].astype(np.float64) @ W1.astype(np.float64).T + b1.astype(np.float64)[None, :]
    mag = np.abs(X[:M].astype(np.float64)) @ np.abs(W1.astype(np.float64)).T + np.abs(b1.astype(np.float64))[None, :]
    chain = (R.gemm_chain(W1, X[:M], R.uniform_ranges(F // 32, lambda s: (0, KB), 1))[0] + b1[None, :]).astype(np.float32)
    ec = float((np.abs(chain - pre) / mag).max())
    if bx:
        val = R.check_planes_consistent(pr.get("hq")[:F // 16 * MT * 3 * 64 * 8], MT, F, M, "hq planes")
    else:
        val = pr.get_act("hbuf", MT, F)
    figs["FC1"] = R.check_gelu(val[:M], pre, "FC1 (%s)" % plan["roles"]["fc1"], pre_tol=R.DENSE_GATE * ec * mag)
    X = rs.standard_normal((32 * MT, D)).astype(np.float32)
    X[M:] = GARBAGE
    pr.sentinel_work()
    pr.put_act("h", X, MT)
    lg = pr.run(R.HEAD, R.HEAD, M, pos=1, layer=pr.nl - 1, want_logits=True)
    W, b = pr.w("lm_head.weight"), pr.w("lm_head.bias")
    ref = X[:M].astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)[None, :]
    mag = np.abs(X[:M].astype(np.float64)) @ np.abs(W.astype(np.float64)).T + np.abs(b.astype(np.float64))[None, :]
    chain = (R.gemm_chain(W, X[:M], R.uniform_ranges(V // 32, lambda s: (0, KB), 1))[0] + b[None, :]).astype(np.float32)
    e, ec = float((np.abs(lg - ref) / mag).max()), float((np.abs(chain - ref) / mag).max())
    assert e <= R.DENSE_GATE * ec, "head: normalised error %.3g is %.2f x the fp32 chain's %.3g" % (e, e / ec, ec)
    _say("dense %s%s M=%d" % (name, "/".join(env), M), qkv=figs["QKV"], proj=figs["PROJ"], fc2=figs["FC2"], adaln=figs["ADALN"], fc1_gelu=figs["FC1"], head=e / ec, bx=bx,
         adaln_k=plan["roles"]["adaln"], fc1_k=plan["roles"]["fc1"])
