"""What survives from one call of a decode engine to the next: captured graphs, and the state an engine carries.

1. The call ladders of tests/call_ladders.py on the device, through the C ABI with caller-held buffers (so that an address changes only
   when a rung says so).  Two engines per model from one synthetic state: the engine under test runs with use_graph = 1, its twin
   eager -- the reference (eager loops are held to the reference's tokens elsewhere, and graph == eager bit for bit is what
   test_gpu_determinism.py and test_gpu_hook.py establish; there are no floating-point atomics).  Per rung: tokens (and the traced
   logits: the fused trace, or what the hook saw) bit-equal to the twin's; the engine's capture counter (wmar_*_graph_counts) moved if
   and only if the rung says MAY_CAPTURE; every output buffer the call did not name is still the -1 it was prefilled with; and the
   twin's own output DIFFERS from its output for the call before on every VALUE rung -- without that a stale graph would pass.
2. History independence: a list of heterogeneous calls per model, in order with graphs on one engine and in reverse order eager on
   another: the result of a call is a function of its arguments, whatever the engine ran before.
3. The key-table cache of gentime_watermark.py: one device table shared by watermarkers that differ in delta only, and eviction.

Every figure line starts with CALLSTATE."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import call_ladders as CL  # noqa: E402
from tests import hook_processors as HP  # noqa: E402
from tests.conftest import load_ids  # noqa: E402
from tests.engine_probe import parse_plan  # noqa: E402
from wmar_amd import _lib  # noqa: E402
from wmar_amd.utils import synth  # noqa: E402

V_GPT = 16384
# production width, two layers; 64 positions, so that the attention-schedule rungs reach cache lengths at which the schedule moves bits
PROD = synth.GPTConfig(vocab_size=V_GPT, block_size=64, n_layer=2, n_head=CL.GPT_HEADS, n_embd=1536)
SMALL = synth.GPTConfig(vocab_size=V_GPT, block_size=16, n_layer=2, n_head=4, n_embd=128)
RCFG = synth.RARConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, image_seq_len=16,
                       codebook_size=1024, condition_num_classes=1000)
CCFG = synth.ChameleonConfig(dim=256, n_layers=2, n_heads=4, n_kv_heads=4, vocab_size=2048, multiple_of=64)
CHAM_T = 32                      # max_seq_len of the Chameleon engines: 7 prompt + 16 image tokens and room to spare


def row_hash_bias(past_ids, logits):
    """hook_processors.hash_bias keyed by the sum of the WHOLE row: every id the hook is shown moves every later step (the class
    token, the left padding of a Chameleon prompt); +8 / -4, so that it still decides tokens at the ladders' temperature"""
    ctx = past_ids.sum(dim=1).to(logits.device)
    ids = torch.arange(logits.shape[1], dtype=torch.int64, device=logits.device)
    r = (ids[None, :] * 2654435761 + ctx[:, None]) % 5
    logits.copy_(torch.where(r == 0, logits + 8.0, torch.where(r == 1, logits - 4.0, logits)))
    return logits


def noise(seed, n):
    return torch.empty(n, device="cuda").exponential_(1, generator=torch.Generator(device="cuda").manual_seed(seed))


class Pool:
    """caller-held device buffers: (name, slot) -> tensor, allocated once and kept, so that two slots never share an address"""

    def __init__(self):
        self.t = {}

    def add(self, name, slots, numel, dtype):
        for s in range(slots):
            self.t[name, s] = torch.empty(numel, dtype=dtype, device="cuda")
        assert len({self.t[name, s].data_ptr() for s in range(slots)}) == slots

    def __getitem__(self, key):
        return self.t[key]

    def slots(self, name):
        return [t for (n, _), t in self.t.items() if n == name]


class Hook:
    """the host side of a hooked call on caller-held buffers: keeps what the processor was shown (the hooked loops' logit trace)"""

    def __init__(self, logits, past, B, V, stride, processor):
        self.logits, self.past = logits[:B * V].view(B, V), past[:B * stride].view(B, stride)
        self.processor, self.seen, self.error = processor, [], None
        self.cfunc = _lib.LOGITS_HOOK(self._call)

    def _call(self, user, step, t):
        try:
            with torch.no_grad():
                if step == 0:
                    del self.seen[:]             # a run repeated behind a barrier fallback starts over
                self.seen.append(self.logits.clone())
                self.processor(self.past[:, :t], self.logits)
            return 0
        except BaseException as e:  # noqa: BLE001  (nothing may cross the C frames)
            self.error = e
            return 1

    def trace(self):
        if self.error is not None:
            raise self.error
        return torch.stack(self.seen)


def _differs(a, b):
    """two results (tuples of tensors): another shape, or another bit"""
    return any(x.shape != y.shape or not torch.equal(x, y) for x, y in zip(a, b)) or len(a) != len(b)


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _where(a, b):
    """where two results differ: per tensor, the first differing index along the first dimension"""
    out = []
    for i, (x, y) in enumerate(zip(a, b)):
        if x.shape != y.shape:
            out.append("#%d shapes %s / %s" % (i, tuple(x.shape), tuple(y.shape)))
        elif not torch.equal(x, y):
            d = (x != y).flatten(1).any(1).nonzero().view(-1).tolist()
            out.append("#%d differs at [%s] of %d (%d elements)" % (i, ",".join(map(str, d[:8])), x.shape[0], int((x != y).sum())))
    return "; ".join(out) or "equal"


def run_ladder(loop, driver):
    """The ladder of `loop` through driver.call(call, graph) -> result (tuple of tensors: tokens, trace), with the per-rung checks every
    keyed loop shares.  The driver also has counts() -> the capture counter of this loop and of the other one, fallbacks() and
    check_untouched(call)."""
    prev_twin = prev_got = None
    for rung, call in CL.calls(loop):
        name = rung.name if rung else "base"
        driver.prepare(call)
        c0, fb0 = driver.counts(), driver.fallbacks()
        got = driver.call(call, graph=True)
        c1, fb1 = driver.counts(), driver.fallbacks()
        driver.check_untouched(call, name)
        driver.prepare(call)
        twin = driver.call(call, graph=False)
        moved = c1[0] - c0[0]
        assert c1[1] == c0[1], f"{loop} {name}: the other loop's graphs were captured"
        equal = _same(got, twin)
        print("CALLSTATE %-11s %-26s captures=%d equal=%d%s" % (loop, name, moved, equal, "" if fb1 == fb0 else " (barrier fallback: counter not held)"))
        assert equal, (f"{loop} {name}: the graph call differs from the eager twin: {_where(got, twin)}; graph call against its own result "
                       f"for the call before: {_where(got, prev_got) if prev_got else '-'}; the twin against its own: "
                       f"{_where(twin, prev_twin) if prev_twin else '-'}")
        prev_got = got
        if fb1 == fb0:
            want = rung is None or rung.expect == CL.MAY_CAPTURE
            assert (moved > 0) == want, f"{loop} {name}: {moved} captures, the ladder says {rung.expect if rung else 'capture'}"
            driver.check_captures(call, name, moved)
        if rung is not None:
            if rung.kind == CL.VALUE:
                assert _differs(twin, prev_twin), f"{loop} {name}: vacuous -- the eager result did not change with {rung.field}"
            else:       # (a trace pointer that comes or goes changes how much there is to compare, not what is computed)
                k = min(len(twin), len(prev_twin))
                assert _same(twin[:k], prev_twin[:k]), f"{loop} {name}: the eager result changed with {rung.field}"
        prev_twin = tuple(t.clone() for t in twin)


# ------------------------------------------------------------------------------------------------------------------- GPT
def _gpt_pair(cfg, max_batch):
    from wmar_amd.models.engine import GPTEngine
    state = synth.synth_gpt_state_fast(cfg, seed=1, device="cuda", logit_scale=10.0)
    return GPTEngine(cfg, state, max_batch=max_batch), GPTEngine(cfg, state, max_batch=max_batch)


@pytest.fixture(scope="module")
def gpt_prod():
    return _gpt_pair(PROD, 128)


def _taming_vq():
    ids = load_ids("vqgan_alive_ids.txt")
    return {"alive_ids": torch.tensor(ids), "dead_ids": torch.tensor(sorted(set(range(V_GPT)) - set(ids))), "embedding": None}


def _taming_wm(delta=2.0, salt=15485863, h=1):
    from wmar_amd.watermarking.gentime_watermark import GentimeWatermark, SeedStrategy, SplitStrategy
    return GentimeWatermark(_taming_vq(), V_GPT, SeedStrategy.LINEAR, SplitStrategy.RANDOM_STRATIFIED, h, delta, 0.25, device="cuda",
                            salt_key=salt)


def gpt_generate_raw(eng, wm_ctx, sp, cond, B, steps, q, out, trace):
    L = _lib.load()
    _lib.check(L.wmar_gpt_generate(eng._h, C.byref(wm_ctx) if wm_ctx is not None else None, C.byref(sp), cond.data_ptr(), B, steps,
                                   q.data_ptr(), out.data_ptr(), trace.data_ptr() if trace is not None else None, _lib.stream_ptr()))
    _lib.check(L.wmar_gpt_check(eng._h, _lib.stream_ptr()))
    torch.cuda.synchronize()


class GptDriver:
    BMAX, SMAX, STRIDE_MAX = 14, 40, 44

    def __init__(self, engines, hooked):
        self.eng, self.twin, self.hooked = engines[0], engines[1], hooked
        self.pool = p = Pool()
        nq = self.SMAX * self.BMAX * V_GPT
        p.add("q", 2, nq, torch.float32)
        p.add("out", 2, self.BMAX * self.SMAX, torch.int64)
        p.add("cond", 1, self.BMAX, torch.int64)
        p.add("t_out", 1, self.BMAX * self.SMAX, torch.int64)
        self.q_src = [noise(31 + i, nq) for i in range(2)]
        self.cond_src = [(torch.arange(self.BMAX) * 37 % 1000).cuda(), ((torch.arange(self.BMAX) * 53 + 7) % 1000).cuda()]
        if hooked:
            p.add("hook_logits", 2, self.BMAX * V_GPT, torch.float32)
            p.add("hook_past", 2, self.BMAX * self.STRIDE_MAX, torch.int64)
            p.add("t_hook_logits", 1, self.BMAX * V_GPT, torch.float32)
            p.add("t_hook_past", 1, self.BMAX * self.STRIDE_MAX, torch.int64)
        else:
            p.add("trace", 2, nq, torch.float32)
            p.add("t_trace", 1, nq, torch.float32)
            p.add("table", 2, CL.N_ROWS_FULL * (V_GPT // 32), torch.int32)
            self.table_src = [torch.from_numpy(_taming_wm(salt=s).key_table_host(CL.N_ROWS_FULL).view(np.int32)).reshape(-1).cuda()
                              for s in (15485863, 32452843)]
            assert not torch.equal(self.table_src[0], self.table_src[1])
        self.state = {"att_phases": None, "timing": 0}

    OUTPUTS = ("out", "trace", "hook_logits", "hook_past")

    def prepare(self, call):
        """contents into the buffers the call names; every output slot (and the twin's) prefilled with -1; engine switches on both"""
        p = self.pool
        p["q", call["q@"]].copy_(self.q_src[call["q#"]])
        p["cond", 0].copy_(self.cond_src[call["cond#"]])
        if not self.hooked:
            p["table", call["table@"]].copy_(self.table_src[call["table#"]])
        for (n, _), t in p.t.items():
            if n in self.OUTPUTS or n.startswith("t_"):
                t.fill_(-1)
        if call["att_phases"] != self.state["att_phases"]:
            for e in (self.eng, self.twin):
                e.set_attention_phases(*(call["att_phases"] or (-1, -1)))
        if call.get("timing", 0) != self.state["timing"]:
            for e in (self.eng, self.twin):
                e.set_timing(bool(call["timing"]))
        self.state = {"att_phases": call["att_phases"], "timing": call.get("timing", 0)}
        torch.cuda.synchronize()

    def counts(self):
        c = self.eng.graph_counts()
        return (c["hooked"], c["fused"]) if self.hooked else (c["fused"], c["hooked"])

    def fallbacks(self):
        return int(self.eng.plan_info(14)["barrier_fallbacks"])

    def call(self, call, graph):
        p, B, steps = self.pool, call["B"], call["steps"]
        eng = self.eng if graph else self.twin
        sp = _lib.SampleParams(call["temperature"], call["top_k"], call["top_p"], 1 if graph else 0)
        out = p["out", call["out@"]] if graph else p["t_out", 0]
        q, cond = p["q", call["q@"]], p["cond", 0]
        if self.hooked:
            stride = call["past_stride"]
            hk = Hook(p["hook_logits", call["hook_logits@"]] if graph else p["t_hook_logits", 0],
                      p["hook_past", call["hook_past@"]] if graph else p["t_hook_past", 0], B, V_GPT, stride, row_hash_bias)
            rc = _lib.load().wmar_gpt_generate_hooked(eng._h, C.byref(sp), cond.data_ptr(), B, steps, q.data_ptr(), out.data_ptr(),
                                                      hk.logits.data_ptr(), hk.past.data_ptr(), stride, hk.cfunc, None, _lib.stream_ptr())
            if hk.error is not None:
                raise hk.error
            _lib.check(rc)
            _lib.check(_lib.load().wmar_gpt_check(eng._h, _lib.stream_ptr()))
            torch.cuda.synchronize()
            toks = out[:B * steps].view(B, steps).clone()
            # the engine appends to the caller's past buffer: class token, then the tokens, at the stride the call gave
            assert torch.equal(hk.past[:, :steps + 1], torch.cat([cond[:B, None], toks], dim=1))
            return toks, hk.trace()
        wm = None
        if call["wm"]:
            wm = _lib.WmCtx(p["table", call["table@"]].data_ptr(), call["n_rows"], V_GPT, call["seed_strategy"], call["context_size"],
                            call["spatial_dim"], call["delta"])
        trace = (p["trace", call["trace@"]] if call["trace@"] is not None else None) if graph else p["t_trace", 0]
        gpt_generate_raw(eng, wm, sp, cond, B, steps, q, out, trace)
        res = (out[:B * steps].view(B, steps).clone(),)
        if call["trace@"] is not None:
            res += (trace[:steps * B * V_GPT].view(steps, B, V_GPT).clone(),)
        return res

    def check_untouched(self, call, name):
        """behind the graph call: the buffers it named are written, every other output slot still holds the -1 it was prefilled with"""
        p, n = self.pool, call["B"] * call["steps"]
        for base in ("out", "trace", "hook_logits", "hook_past"):
            if (base, 0) not in p.t:
                continue
            used = call[base + "@"]
            for s in (0, 1):
                t = p[base, s]
                if s == used:
                    assert bool((t[:n] != -1).all()) if base == "out" else bool((t != -1).any()), f"{name}: {base}@{s} was not written"
                else:
                    assert bool((t == -1).all()), f"{name}: {base}@{s} was written, the call names {base}@{used}"
        for t in p.slots("t_out") + p.slots("t_trace") + p.slots("t_hook_logits") + p.slots("t_hook_past"):
            assert bool((t == -1).all()), f"{name}: the graph call wrote a buffer of the eager twin"

    def check_captures(self, call, name, moved):
        """the rung reached the branch it names: the plan of its batch, and one capture per graph slot its steps pass through"""
        small = "path" in self.eng.plan_info(call["B"])
        assert small == (call["B"] <= 12), (name, call["B"])
        if moved:
            assert moved == len(CL.gpt_slots(call, self.hooked)), (name, moved, CL.gpt_slots(call, self.hooked))
        if call["att_phases"] == (2, 4):
            assert "(1 / 4 / 4 waves" in self.eng.plan_info(call["B"])["attn"], self.eng.plan_info(call["B"])["attn"]


def test_gpt_fused_ladder(gpt_prod):
    run_ladder("gpt_fused", GptDriver(gpt_prod, hooked=False))


def test_gpt_hooked_ladder(gpt_prod):
    run_ladder("gpt_hooked", GptDriver(gpt_prod, hooked=True))


# ------------------------------------------------------------------------------------------------------------------- RAR
def _rar_engine():
    from wmar_amd.models.engine import RAREngine
    return RAREngine(RCFG, synth.synth_rar_state(RCFG, seed=2, logit_scale=30.0), max_batch=8)


@pytest.fixture(scope="module")
def rar_pair():
    return _rar_engine(), _rar_engine()


class RarDriver:
    BMAX, L, V, STRIDE_MAX = 8, 16, 1024, 19

    def __init__(self, engines):
        self.eng, self.twin = engines
        self.pool = p = Pool()
        nq = self.L * self.BMAX * self.V
        p.add("q", 2, nq, torch.float32)
        p.add("cls", 1, self.BMAX, torch.int64)
        for pre in ("", "t_"):
            n = 2 if not pre else 1
            p.add(pre + "out", n, self.BMAX * self.L, torch.int64)
            p.add(pre + "hook_logits", n, self.BMAX * self.V, torch.float32)
            p.add(pre + "hook_past", n, self.BMAX * self.STRIDE_MAX, torch.int64)
        self.q_src = [noise(41 + i, nq) for i in range(2)]
        self.cls_src = [((torch.arange(self.BMAX) * 13 + 3) % 1000).cuda(), ((torch.arange(self.BMAX) * 29 + 11) % 1000).cuda()]
        ramp = np.arange(self.L, dtype=np.float32) / (self.L - 1)
        self.scale_src = [1 + 3 * ramp, 4 - 3 * ramp]
        self.scales = np.zeros(self.L, dtype=np.float32)               # the ONE host array every call passes

    def prepare(self, call):
        p = self.pool
        p["q", call["q@"]].copy_(self.q_src[call["q#"]])
        p["cls", 0].copy_(self.cls_src[call["class#"]])
        self.scales[:] = self.scale_src[call["cfg_scales#"]]
        for (n, _), t in p.t.items():
            if n not in ("q", "cls"):
                t.fill_(-1)
        torch.cuda.synchronize()

    def counts(self):
        c = self.eng.graph_counts()
        return c["hooked"], c["fused"]

    def fallbacks(self):
        return self.eng.launch_status()["fallbacks"]

    def call(self, call, graph):
        p = self.pool
        guided, B = CL.rar_rows(call["rows"])
        eng, stride = (self.eng if graph else self.twin), call["past_stride"]
        out = p["out", call["out@"]] if graph else p["t_out", 0]
        hk = Hook(p["hook_logits", call["hook_logits@"]] if graph else p["t_hook_logits", 0],
                  p["hook_past", call["hook_past@"]] if graph else p["t_hook_past", 0], B, self.V, stride, row_hash_bias)
        L = _lib.load()
        rc = L.wmar_rar_generate_hooked(eng._h, p["cls", 0].data_ptr(), B, self.scales.ctypes.data_as(C.POINTER(C.c_float)), int(guided),
                                        call["temperature"], p["q", call["q@"]].data_ptr(), out.data_ptr(), 1 if graph else 0,
                                        hk.logits.data_ptr(), hk.past.data_ptr(), stride, hk.cfunc, None, _lib.stream_ptr())
        if hk.error is not None:
            raise hk.error
        _lib.check(rc)
        _lib.check(L.wmar_rar_check(eng._h, _lib.stream_ptr()))
        torch.cuda.synchronize()
        toks = out[:B * self.L].view(B, self.L).clone()
        assert torch.equal(hk.past[:, :self.L], toks)
        return toks, hk.trace()

    def check_untouched(self, call, name):
        p = self.pool
        _, B = CL.rar_rows(call["rows"])
        for base in ("out", "hook_logits", "hook_past"):
            for s in (0, 1):
                t = p[base, s]
                if s == call[base + "@"]:
                    assert bool((t[:B * self.L] != -1).all()) if base == "out" else bool((t != -1).any()), f"{name}: {base}@{s} was not written"
                else:
                    assert bool((t == -1).all()), f"{name}: {base}@{s} was written, the call names {base}@{call[base + '@']}"
        for base in ("t_out", "t_hook_logits", "t_hook_past"):
            assert bool((p[base, 0] == -1).all()), f"{name}: the graph call wrote a buffer of the eager twin"

    def check_captures(self, call, name, moved):
        guided, B = CL.rar_rows(call["rows"])
        M = 2 * B if guided else B
        buf = C.create_string_buffer(4096)
        _lib.check(_lib.load().wmar_rar_probe_plan(self.eng._h, M, B, int(guided), 1, buf, len(buf)))
        plan = parse_plan(buf.value.decode())
        assert plan["MT"] == 1 and plan["MTc"] == 1, plan             # g2 and u4: the same four rows, told apart by the key alone
        if moved:
            assert moved == 2, (name, moved)                          # the position's graph and the sampler's


def test_rar_hooked_ladder(rar_pair):
    run_ladder("rar_hooked", RarDriver(rar_pair))


# ------------------------------------------------------------------------------------------------------------- Chameleon
def _cham_engine():
    from wmar_amd.models.engine import ChameleonEngine
    return ChameleonEngine(CCFG, synth.synth_chameleon_state(CCFG, seed=8, logit_scale=6.0), max_batch=3, max_seq_len=CHAM_T)


@pytest.fixture(scope="module")
def cham_pair():
    return _cham_engine(), _cham_engine()


def _t(i):
    return 520 + (i * 37) % 1500            # a "text" id of the 2048-entry vocabulary (image ids: 4 .. 515)


# three prompts of unequal length per variant (full-conditioned stream); the image-conditioned stream keeps the last id, the
# unconditioned one is a single id.  Variant 0: the longest row has 5 ids, variant 1: 7.
CHAM_PROMPTS = [
    [[_t(1), _t(2), _t(3)], [_t(4)], [_t(5), _t(6), _t(7), _t(8), _t(9)]],
    [[_t(11), _t(12)], [_t(13), _t(14), _t(15), _t(16), _t(17), _t(18), _t(19)], [_t(20), _t(21), _t(22), _t(23)]],
]
CHAM_ALLOW = [list(range(4, 516)), list(range(300, 900))]


def cham_prompts(variant, B):
    full = CHAM_PROMPTS[variant][:B]
    return full + [p[-1:] for p in full] + [[_t(40)] for _ in full]


class ChamDriver:
    BMAX, NMAX, V, STRIDE_MAX = 3, 16, 2048, 27

    def __init__(self, engines):
        from wmar_amd.models.chameleon_wrapper import allow_bitmap
        self.eng, self.twin = engines
        self.pool = p = Pool()
        nq = self.NMAX * self.BMAX * self.V
        p.add("q", 2, nq, torch.float32)
        p.add("allow", 2, self.V // 32, torch.int32)
        p.add("allow_ids", 1, self.V, torch.int32)
        for pre in ("", "t_"):
            n = 2 if not pre else 1
            p.add(pre + "out", n, self.BMAX * self.NMAX, torch.int64)
            p.add(pre + "hook_logits", n, self.BMAX * self.V, torch.float32)
            p.add(pre + "hook_past", n, self.BMAX * self.STRIDE_MAX, torch.int64)
        self.q_src = [noise(51 + i, nq) for i in range(2)]
        self.allow_src = [allow_bitmap(ids, self.V, "cuda") for ids in CHAM_ALLOW]
        # the host arrays every call passes: lengths and tokens are rewritten in place
        self.tok = np.zeros(64, dtype=np.int64)
        self.lens = np.zeros(3 * self.BMAX, dtype=np.int32)

    def prepare(self, call):
        p = self.pool
        p["q", call["q@"]].copy_(self.q_src[call["q#"]])
        p["allow", call["allow@"]].copy_(self.allow_src[call["allow#"]])
        ids = CHAM_ALLOW[call["allow#"]]
        p["allow_ids", 0][:len(ids)].copy_(torch.tensor(ids, dtype=torch.int32))
        self.n_allow = len(ids)
        prompts = cham_prompts(call["prompts#"], call["B"])
        flat = np.concatenate([np.asarray(q, dtype=np.int64) for q in prompts])
        self.tok[:] = 0
        self.tok[:len(flat)] = flat
        self.lens[:] = 0
        self.lens[:len(prompts)] = [len(q) for q in prompts]
        self.maxlen = max(len(q) for q in prompts)
        assert min(len(q) for q in prompts[:call["B"]]) < self.maxlen          # a first-stream row is left-padded: pad_id is seen
        for (n, _), t in p.t.items():
            if n.startswith(("out", "hook_", "t_")):
                t.fill_(-1)
        torch.cuda.synchronize()

    def counts(self):
        c = self.eng.graph_counts()
        return c["hooked"], c["fused"]

    def fallbacks(self):
        return 0                         # this engine has no in-launch barrier

    def call(self, call, graph):
        p, B, n = self.pool, call["B"], call["n_tokens"]
        eng, stride = (self.eng if graph else self.twin), call["past_stride"]
        out = p["out", call["out@"]] if graph else p["t_out", 0]
        hk = Hook(p["hook_logits", call["hook_logits@"]] if graph else p["t_hook_logits", 0],
                  p["hook_past", call["hook_past@"]] if graph else p["t_hook_past", 0], B, self.V, stride, row_hash_bias)
        sp = _lib.ChamSampleParams(call["temperature"], call["top_p"], call["g_text"], call["g_image"], 1 if graph else 0, call["pad_id"])
        comp = call["compaction"]
        rc = _lib.load().wmar_cham_generate_image_hooked(
            eng._h, self.tok.ctypes.data, self.lens.ctypes.data, B, C.byref(sp), p["allow", call["allow@"]].data_ptr(),
            p["allow_ids", 0].data_ptr() if comp else None, self.n_allow if comp else 0, p["q", call["q@"]].data_ptr(), n, out.data_ptr(),
            hk.logits.data_ptr(), hk.past.data_ptr(), stride, hk.cfunc, None, _lib.stream_ptr())
        if hk.error is not None:
            raise hk.error
        _lib.check(rc)
        torch.cuda.synchronize()
        toks = out[:B * n].view(B, n).clone()
        # the caller's past buffer: the first stream's prompts left-padded with pad_id, then the tokens
        rows = [[call["pad_id"]] * (self.maxlen - len(q)) + q for q in cham_prompts(call["prompts#"], B)[:B]]
        assert torch.equal(hk.past[:, :self.maxlen + n], torch.cat([torch.tensor(rows).cuda(), toks], dim=1))
        allowed = set(CHAM_ALLOW[call["allow#"]])
        assert set(toks.flatten().tolist()) <= allowed
        return toks, hk.trace()

    def check_untouched(self, call, name):
        p, n = self.pool, call["B"] * call["n_tokens"]
        for base in ("out", "hook_logits", "hook_past"):
            for s in (0, 1):
                t = p[base, s]
                if s == call[base + "@"]:
                    assert bool((t[:n] != -1).all()) if base == "out" else bool((t != -1).any()), f"{name}: {base}@{s} was not written"
                else:
                    assert bool((t == -1).all()), f"{name}: {base}@{s} was written, the call names {base}@{call[base + '@']}"
        for base in ("t_out", "t_hook_logits", "t_hook_past"):
            assert bool((p[base, 0] == -1).all()), f"{name}: the graph call wrote a buffer of the eager twin"

    def check_captures(self, call, name, moved):
        buf = C.create_string_buffer(4096)
        _lib.check(_lib.load().wmar_cham_probe_plan(self.eng._h, 3 * call["B"], buf, len(buf)))
        assert parse_plan(buf.value.decode(), list_keys=(), ints=False)["MT"] == "1"
        if moved:
            assert moved == 2, (name, moved)                          # the model step's graph (steps 1 ..) and the sampler's


def test_cham_hooked_ladder(cham_pair):
    run_ladder("cham_hooked", ChamDriver(cham_pair))


# --------------------------------------------------------------------------------------------------- history independence
def run_histories(name, calls, first, second, fresh=None):
    """calls: [(tag, f(engine, graph) -> tuple of tensors)].  `first` runs them in order with graphs, `second` in reverse order eager;
    every call's result must be the same bits on both.  fresh: a factory -- the first, a middle and the last call also run on an engine
    created for that call alone."""
    a = {tag: tuple(t.clone() for t in f(first, True)) for tag, f in calls}
    b = {tag: tuple(t.clone() for t in f(second, False)) for tag, f in reversed(calls)}
    for tag, _ in calls:
        ok = _same(a[tag], b[tag])
        print("CALLSTATE %-11s %-26s in_order_graph == reversed_eager: %d" % (name, tag, ok))
        assert ok, f"{name} {tag}: the result depends on what the engine ran before"
    if fresh is not None:
        for i in (0, len(calls) // 2, len(calls) - 1):
            tag, f = calls[i]
            e = fresh()
            ok = _same(tuple(t.clone() for t in f(e, True)), a[tag])
            del e
            print("CALLSTATE %-11s %-26s fresh engine == in_order_graph: %d" % (name, tag, ok))
            assert ok, f"{name} {tag}: differs from an engine created for this call alone"


def gpt_history(V=V_GPT):
    wm = _taming_wm()

    def gen(B, steps=16, wmk=False, hooked=False, seed=0, trace=False, phases=None):
        def f(e, graph):
            cond = ((torch.arange(B) * 37 + seed) % 1000).cuda()
            q = noise(60 + seed + B, steps * B * V).view(steps, B, V)
            if phases:
                e.set_attention_phases(*phases)
            try:
                if hooked:
                    return (e.generate_hooked(cond, steps, q, HP.hash_bias, 1.0, 250, 0.92, use_graph=graph),)
                r = e.generate(cond, steps, q, 1.0, 250, 0.92, wm.wm_ctx() if wmk else None, use_graph=graph, trace_logits=trace)
                return r if trace else (r,)
            finally:
                if phases:
                    e.set_attention_phases(-1, -1)
        return f

    def steps_127(e, graph):
        tok = torch.randint(0, V, (3, 127), generator=torch.Generator().manual_seed(8)).cuda()
        return tuple(e.decode_step(tok[p], p) for p in range(3))

    return [("generate_B64_wm", gen(64, wmk=True, trace=True)), ("decode_step_127_rows", steps_127), ("generate_B5", gen(5, trace=True)),
            ("hooked_B13", gen(13, hooked=True)), ("generate_B33_steps7", gen(33, steps=7)), ("generate_B1", gen(1)),
            ("phases_2_4_generate_B64", gen(64, seed=3, phases=(2, 4))), ("generate_B128_steps4", gen(128, steps=4)),
            ("generate_B12_wm", gen(12, wmk=True, seed=5))]


def test_gpt_results_do_not_depend_on_history_production_width(gpt_prod):
    first, second = gpt_prod
    run_histories("gpt_prod", gpt_history(), first, second)
    assert "k_sgemv" in first.plan_info(5)["qkv"] and "path" not in first.plan_info(13)       # the list crosses the small-batch plan


def test_gpt_results_do_not_depend_on_history_small_config():
    from wmar_amd.models.engine import GPTEngine
    state = synth.synth_gpt_state(SMALL, seed=3, logit_scale=10.0)

    def make():
        return GPTEngine(SMALL, state, max_batch=128)
    run_histories("gpt_small", gpt_history(), make(), make(), fresh=make)


def rar_history():
    L, V = RCFG.image_seq_len, RCFG.codebook_size
    ramp = torch.arange(L, dtype=torch.float32) / (L - 1)

    def args(B, seed):
        return ((torch.arange(B) * 13 + seed) % 1000).cuda(), noise(70 + seed + B, L * B * V).view(L, B, V)

    def gen(B, guided, seed=0, hooked=False, T=1.0):
        def f(e, graph):
            cls, q = args(B, seed)
            sc = (1 + 3 * ramp) if guided else None
            if hooked:
                return (e.generate_hooked(cls, q, sc, HP.hash_bias, T, use_graph=graph),)
            return (e.generate(cls, q, sc, T, None, use_graph=graph),)
        return f

    def gumbel(e, graph):
        cls, _ = args(3, 1)
        log_rs = torch.rand(V, generator=torch.Generator().manual_seed(9)).clamp_min(1e-6).log().cuda()
        return (e.generate_gumbel(cls, log_rs, 1 + 3 * ramp, 1.0, 0.0, 0, use_graph=graph),)

    def gumbel_ctx(e, graph):
        cls, _ = args(4, 2)
        u = torch.rand(2, 4, V, generator=torch.Generator().manual_seed(10)).clamp_min(1e-6).cuda()
        return (e.generate_gumbel_ctx(cls, 123456789, 2, u, 1 + 3 * ramp, 1.0, 0.0, 0, use_graph=graph),)

    def position_5(e, graph):
        """positions 0 .. 5 of three rows: position 5 reads the cache rows this call wrote, whatever lay there before"""
        cond = (torch.tensor([5, 700, 31]) + V + 1).cuda()
        toks = torch.randint(0, V, (6, 3), generator=torch.Generator().manual_seed(11)).cuda()
        e.forward_position(torch.full((3,), -1, dtype=torch.int64).cuda(), cond, 0)
        for pos in range(1, 5):
            e.forward_position(toks[pos], cond, pos)
        return (e.forward_position(toks[5], cond, 5),)

    return [("generate_guided_B4", gen(4, True)), ("generate_unguided_B8", gen(8, False, seed=1)), ("generate_gumbel", gumbel),
            ("generate_gumbel_ctx_ngram2", gumbel_ctx), ("forward_position_5_M3", position_5),
            ("hooked_guided_B2", gen(2, True, seed=2, hooked=True)), ("hooked_unguided_B4", gen(4, False, seed=3, hooked=True)),
            ("generate_guided_B8_T07", gen(8, True, seed=4, T=0.7))]


def test_rar_results_do_not_depend_on_history(rar_pair):
    run_histories("rar_small", rar_history(), rar_pair[0], rar_pair[1], fresh=_rar_engine)
    assert rar_pair[0].launch_status()["fallbacks"] == 0


def cham_history():
    from wmar_amd.models.chameleon_wrapper import allow_bitmap
    V = CCFG.vocab_size
    long_p = [[_t(60 + i) for i in range(9)], [_t(70 + i) for i in range(6)], [_t(80 + i) for i in range(11)]]
    short_p = [[_t(90)], [_t(91), _t(92)], [_t(93)]]

    def split(full):
        return full + [p[-1:] for p in full] + [[_t(40)] for _ in full]

    def gen(full, n, seed, comp=None, hooked=False):
        def f(e, graph):
            B = len(full)
            q = noise(80 + seed, n * B * V).view(n, B, V)
            kw = {}
            if comp is not None:
                kw["allow"] = allow_bitmap(CHAM_ALLOW[0], V, "cuda")
                if comp:
                    kw["allow_ids"] = torch.tensor(CHAM_ALLOW[0], dtype=torch.int32).cuda()
            if hooked:
                return (e.generate_image_hooked(split(full), q, n, HP.hash_bias, 0.9, 0.8, 3.0, 1.2, use_graph=graph, **kw),)
            return (e.generate_image(split(full), q, n, 0.9, 0.8, 3.0, 1.2, use_graph=graph, **kw),)
        return f

    def ragged(e, graph):
        """nine rows: positions 0 .. 2 for all of them, then a step at unequal positions -- every cache row read was written here"""
        tok = torch.randint(0, V, (4, 9), generator=torch.Generator().manual_seed(12)).cuda()
        for pos in range(3):
            e.forward_tokens(tok[pos], torch.full((9,), pos, dtype=torch.int32), want_logits=False)
        return (e.forward_tokens(tok[3], torch.tensor([3, 1, 2, 3, 0, 2, 1, 3, 2], dtype=torch.int32)),)

    return [("generate_long_prompts", gen(long_p, 8, 0)), ("generate_short_prompts", gen(short_p, 8, 1)), ("forward_tokens_ragged", ragged),
            ("generate_n5", gen(long_p[:2], 5, 2)), ("generate_n12", gen(short_p, 12, 3)), ("hooked_n8", gen(long_p, 8, 4, hooked=True)),
            ("generate_compaction", gen(long_p, 8, 5, comp=True)), ("generate_allow_only", gen(long_p, 8, 5, comp=False))]


def test_cham_results_do_not_depend_on_history(cham_pair):
    calls = cham_history()
    run_histories("cham_small", calls, cham_pair[0], cham_pair[1])
    # the compacted sampler row is exact: the two last calls differ in compaction alone
    a, b = (dict(calls)[k](cham_pair[0], True)[0] for k in ("generate_compaction", "generate_allow_only"))
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------ key-table cache
def _cache_run(engines, wm, bufs, graph):
    eng = engines[0] if graph else engines[1]
    B, steps = 14, 16
    q, cond, out = bufs
    out.fill_(-1)
    sp = _lib.SampleParams(1.0, 250, 0.92, 1 if graph else 0)
    gpt_generate_raw(eng, wm.wm_ctx(), sp, cond, B, steps, q, out, None)
    return out.view(B, steps).clone()


@pytest.fixture(scope="module")
def cache_bufs():
    B, steps = 14, 16
    return noise(90, steps * B * V_GPT), ((torch.arange(B) * 37 + 1) % 1000).cuda(), torch.empty(B * steps, dtype=torch.int64, device="cuda")


def test_watermarkers_that_differ_in_delta_share_a_table_and_not_a_graph(gpt_prod, cache_bufs):
    """equal table pointer, equal buffers, another delta: the one case where only a scalar of the watermark tells two calls apart"""
    from wmar_amd.watermarking import gentime_watermark as GW
    GW.clear_key_cache()
    wa, wb = _taming_wm(delta=2.0), _taming_wm(delta=4.0)
    assert wa.key_table().data_ptr() == wb.key_table().data_ptr() and len(GW._TABLE_CACHE) == 1
    c0 = gpt_prod[0].graph_counts()["fused"]
    got = []
    for rep in range(2):
        for tag, wm in (("delta_2", wa), ("delta_4", wb)):
            toks = _cache_run(gpt_prod, wm, cache_bufs, True)
            c1 = gpt_prod[0].graph_counts()["fused"]
            equal = torch.equal(toks, _cache_run(gpt_prod, wm, cache_bufs, False))
            print("CALLSTATE %-11s %-26s captures=%d equal=%d" % ("table_cache", "%s_round%d" % (tag, rep), c1 - c0, equal))
            assert equal and c1 > c0, (tag, rep)
            c0 = c1
            got.append(toks)
    assert not torch.equal(got[0], got[1]) and torch.equal(got[0], got[2]) and torch.equal(got[1], got[3])


def test_a_key_evicted_from_the_table_cache_comes_back_with_the_same_tokens(gpt_prod, cache_bufs):
    """five salts through the four-entry cache, then the first again: its table is rebuilt (perhaps where another one lay, under graphs
    that were captured with that address) -- tokens and p-values as after clear_key_cache()"""
    from wmar_amd.watermarking import gentime_watermark as GW
    GW.clear_key_cache()
    salts = [15485863, 32452843, 49979687, 67867967, 86028121]
    toks = {}
    for s in salts:
        wm = _taming_wm(salt=s)
        toks[s] = _cache_run(gpt_prod, wm, cache_bufs, True)
        assert torch.equal(toks[s], _cache_run(gpt_prod, wm, cache_bufs, False)), s
        del wm
    assert len(GW._TABLE_CACHE) == GW._TABLE_CACHE_MAX and len({t.data_ptr() for t in GW._TABLE_CACHE.values()}) == GW._TABLE_CACHE_MAX
    assert len({tuple(t.flatten().tolist()) for t in toks.values()}) == len(salts)
    first = _taming_wm(salt=salts[0])
    assert first._cache_key() not in GW._TABLE_CACHE                       # evicted: the run below rebuilds it
    again = _cache_run(gpt_prod, first, cache_bufs, True)
    pv_again = first.detect(again)
    GW.clear_key_cache()
    clean_wm = _taming_wm(salt=salts[0])
    clean = _cache_run(gpt_prod, clean_wm, cache_bufs, True)
    pv_clean = clean_wm.detect(clean)
    print("CALLSTATE %-11s %-26s equal=%d pvalue_bits_equal=%d" % ("table_cache", "evicted_key_again", torch.equal(again, clean),
                                                                   torch.equal(pv_again.view(torch.int64), pv_clean.view(torch.int64))))
    assert torch.equal(again, toks[salts[0]]) and torch.equal(again, clean)
    assert torch.equal(again, _cache_run(gpt_prod, clean_wm, cache_bufs, False))
    assert torch.equal(pv_again.view(torch.int64), pv_clean.view(torch.int64))
