"""The call ladders (tests/call_ladders.py) against a host model of keyed graph reuse: do the ladders bite?

The model is what gen_loop.h's ensure_graphs does with an engine's GraphKey, with the launches replaced by "the result is the call's
fields": a call whose key equals the held one (and whose slots all hold a graph) returns f(live fields of this call + BAKED fields of the
call that captured), any other call captures and returns f(this call).  A field is baked when a launch takes it by value -- scalars and
pointers; what a pointer points at, and what a call stages on the host in front of the loop (conditioning ids, prompts, pad_id, guidance
scales), is live.  The eager result is f(this call).

The key words and the baked fields of the four keyed loops are written down here a second time, from reading one_step / step_a / step_b
in gpt.hip, rar.hip and cham.hip -- in call fields: where an engine's key holds a derived word, the model holds what it is derived from.

    gpt.hip   fused   B, steps | gs << 32, q, tokens_out, trace, table (null without wm), n_rows, strategy << 40 | context << 20 |
                      spatial_dim, delta, temperature, top_k, top_p           (gs follows steps and the attention schedule)
    gpt.hip   hooked  B, steps, q, tokens_out, hook logits, hook past, past_stride, temperature, top_k, top_p
    rar.hip   hooked  M, B, q, tokens_out, hook logits, hook past, past_stride, temperature, shared_u, rm_fused
                      (M, B, shared_u follow the ladder's `rows` and no rung can isolate one of them; rm_fused is engine state: REDUNDANT)
    cham.hip  hooked  B, n_tokens, q, tokens_out, hook logits, hook past, ids_stride, allow, allow_ids, n_allow, temperature, top_p,
                      guidance_scale_text, guidance_scale_image              (allow_ids, n_allow: the ladder's `compaction`, see REDUNDANT)
"""
import pytest

from tests import call_ladders as CL

# loop -> {key word: the call fields it is made of}
KEY_WORDS = {
    "gpt_fused": {"B": ["B"], "steps_gs": ["steps"], "q": ["q@"], "tokens_out": ["out@"], "trace": ["trace@"], "table": ["wm", "table@"],
                  "n_rows": ["wm", "n_rows"], "strategy_context_dim": ["wm", "seed_strategy", "context_size", "spatial_dim"],
                  "delta": ["wm", "delta"], "temperature": ["temperature"], "top_k": ["top_k"], "top_p": ["top_p"]},
    "gpt_hooked": {"B": ["B"], "steps": ["steps"], "q": ["q@"], "tokens_out": ["out@"], "hook_logits": ["hook_logits@"],
                   "hook_past": ["hook_past@"], "past_stride": ["past_stride"], "temperature": ["temperature"], "top_k": ["top_k"],
                   "top_p": ["top_p"]},
    "rar_hooked": {"M": ["rows"], "B": ["rows"], "shared_u": ["rows"], "q": ["q@"], "tokens_out": ["out@"], "hook_logits": ["hook_logits@"],
                   "hook_past": ["hook_past@"], "past_stride": ["past_stride"], "temperature": ["temperature"]},
    "cham_hooked": {"B": ["B"], "n_tokens": ["n_tokens"], "q": ["q@"], "tokens_out": ["out@"], "hook_logits": ["hook_logits@"],
                    "hook_past": ["hook_past@"], "ids_stride": ["past_stride"], "allow": ["allow@"], "allow_ids": ["compaction"], "n_allow": ["compaction"],
                    "temperature": ["temperature"], "top_p": ["top_p"], "guidance_scale_text": ["g_text"],
                    "guidance_scale_image": ["g_image"]},
}
# key words that are a function of their fields, not the fields themselves
DERIVED = {
    ("rar_hooked", "M"): lambda c: (2 if CL.rar_rows(c["rows"])[0] else 1) * CL.rar_rows(c["rows"])[1],
    ("rar_hooked", "B"): lambda c: CL.rar_rows(c["rows"])[1],
    ("rar_hooked", "shared_u"): lambda c: CL.rar_rows(c["rows"])[0],
}
# Key words no rung can isolate, because the entry point derives them together: any two of RAR's M, B and shared_u give the third
# (M = 2 B under guidance, M = B without), and Chameleon's allow_ids and n_allow come and go together (the one ids buffer of the test).
# Deleting ONE word of such a group is caught by nothing -- the others still tell the calls apart -- and the test below holds that to be so;
# deleting the whole group is caught, and so is deleting any two of RAR's three, whichever word is kept.  rar.hip's rm_fused is no call field at all: only a barrier
# fallback changes it, which drops the graphs itself (rar_sync_failed), so no ladder can move it.
REDUNDANT = {"rar_hooked": [("M", "B", "shared_u")], "cham_hooked": [("allow_ids", "n_allow")]}
# loop -> the call fields its one_step / step_a / step_b lambdas bake into a launch
BAKED = {
    # enqueue_step(g, B, io): B.  launch_sample_fused(a): make_wm(wm) (table, n_rows, seed_mode, h, S, delta, enabled), temperature, q,
    # q_step_stride = B * V, tok_out, tok_out_stride = steps, top_k, top_p (use_top_p, top_p_thr), trace.
    "gpt_fused": ["B", "steps", "q@", "out@", "trace@", "wm", "table@", "n_rows", "seed_strategy", "context_size", "spatial_dim", "delta",
                  "temperature", "top_k", "top_p"],
    # step_a: enqueue_step(g, B, io{hk.past, pstride, 1, hk.logits}).  step_b: the sampler on hk.logits / hk.past, as above without wm.
    "gpt_hooked": ["B", "steps", "q@", "out@", "hook_logits@", "hook_past@", "past_stride", "temperature", "top_k", "top_p"],
    # step_a: RarPlan(g, M, B, .., shared_u) with ids = hk.past / past_stride, the position's logits -> hk.logits (through k_cfg_mix under
    # guidance).  step_b: the sampler on hk.logits / hk.past, temperature, q, tokens_out.
    "rar_hooked": ["rows", "q@", "out@", "hook_logits@", "hook_past@", "past_stride", "temperature"],
    # step_a: k_cham_step(.., tokens_out, n_tokens, .., B), ChamPlan(g, 3 B), k_cfg_mix(B, g_text, g_image -> hk.logits).  step_b: the
    # sampler on hk.logits / hk.past / ids_stride, temperature, top_p, q, tokens_out, n_tokens, allow, gather = allow_ids / n_allow.
    "cham_hooked": ["B", "n_tokens", "q@", "out@", "hook_logits@", "hook_past@", "past_stride", "temperature", "top_p", "g_text", "g_image",
                    "allow@", "compaction"],
}
# engine switches: wmar_gpt_set_attention_phases drops the FUSED graphs when the schedule changes; wmar_gpt_set_timing drops nothing
DROPS_ON = {"gpt_fused": ["att_phases"], "gpt_hooked": [], "rar_hooked": [], "cham_hooked": []}


def word_value(call, fields, derived=None):
    """a key word's value: its fields; the watermark words are null / 0 without a watermark (key.ptr(wm ? wm->table_dev : nullptr) ...)"""
    if derived is not None:
        return derived(call)
    if "wm" in fields:
        return tuple(call[f] for f in fields if f != "wm") if call["wm"] else None
    return tuple(call[f] for f in fields)


def slots_of(loop, call):
    if loop.startswith("gpt"):
        return CL.gpt_slots(call, hooked=loop == "gpt_hooked")
    return {0, "B"}


class KeyedReuse:
    """the ten-line model: held key, slots that hold a graph, the baked fields of the call that captured"""

    def __init__(self, loop, words):
        self.loop, self.words, self.key, self.slots, self.baked, self.last, self.captures = loop, words, None, set(), {}, None, 0

    def call(self, c):
        if self.last is not None and any(c[f] != self.last[f] for f in DROPS_ON[self.loop]):
            self.slots = set()                                   # the engine dropped its graphs when the switch moved
        key, need = {w: word_value(c, f, DERIVED.get((self.loop, w))) for w, f in self.words.items()}, slots_of(self.loop, c)
        if key != self.key or not need <= self.slots:            # ensure_graphs: drop everything, capture what this call needs
            self.key, self.slots, self.baked = key, set(need), {f: c[f] for f in BAKED[self.loop]}
            self.captures += len(need)
        self.last = c
        return {**c, **self.baked}                               # contents and host-staged fields are read at replay time


def run_model(loop, words):
    """[(rung, captured?, result equals the eager result?)] over the ladder"""
    m, out = KeyedReuse(loop, words), []
    for rung, c in CL.calls(loop):
        before = m.captures
        got = m.call(c)
        out.append((rung, m.captures > before, got == c))
    return out


@pytest.mark.parametrize("loop", list(CL.LADDERS))
def test_every_rung_changes_exactly_one_field(loop):
    cs = CL.calls(loop)
    assert set(cs[0][1]) == set(CL.LADDERS[loop]["base"])
    names = [r.name for r, _ in cs[1:]]
    assert len(set(names)) == len(names), "rung names are the rows of the DESIGN.md table: unique"
    for (_, prev), (rung, cur) in zip(cs, cs[1:]):
        changed = [f for f in cur if cur[f] != prev[f]]
        assert rung.expect in (CL.MUST_REUSE, CL.MAY_CAPTURE) and rung.kind in (CL.VALUE, CL.ADDRESS, CL.NEUTRAL)
        if rung.name == "repeat":
            assert changed == [] and rung.expect == CL.MUST_REUSE and rung.kind == CL.NEUTRAL
        else:
            assert changed == [rung.field], (loop, rung.name, changed)
        if rung.kind == CL.ADDRESS:
            assert rung.field.endswith("@") or rung.field == "past_stride", (loop, rung.name)
    if CL.LADDERS[loop]["keyed"]:
        assert cs[1][0].name == "repeat", "the first rung is the exact repeat: without it every reuse assertion could be vacuous"
    else:
        assert len(cs) == 1


@pytest.mark.parametrize("loop", CL.KEYED)
def test_every_baked_field_is_changed_by_some_rung(loop):
    changed = {r.field for r in CL.LADDERS[loop]["rungs"] if r.name != "repeat"}
    assert set(BAKED[loop]) <= set(CL.LADDERS[loop]["base"])
    assert not set(BAKED[loop]) - changed, sorted(set(BAKED[loop]) - changed)
    # ... and every field a key word is made of is a baked one: the key holds nothing that no launch reads
    assert {f for fs in KEY_WORDS[loop].values() for f in fs} <= set(BAKED[loop])


@pytest.mark.parametrize("loop", CL.KEYED)
def test_full_key_is_exact_and_every_single_word_deletion_is_caught(loop):
    full = run_model(loop, KEY_WORDS[loop])
    assert all(equal for _, _, equal in full), [r.name for r, _, equal in full if not equal]
    # the model's captures are the ladder's expectations: the counter moves if and only if the rung says MAY_CAPTURE
    assert full[0][1]
    for rung, captured, _ in full[1:]:
        assert captured == (rung.expect == CL.MAY_CAPTURE), (loop, rung.name, captured)
    def without(gone):
        rest = {k: v for k, v in KEY_WORDS[loop].items() if k not in gone}
        return [r.name for r, _, equal in run_model(loop, rest) if not equal]

    grouped = {w for g in REDUNDANT.get(loop, []) for w in g}
    caught = {w: without({w}) for w in KEY_WORDS[loop]}
    print("\n".join("KEYWORD %s %-22s caught by %s" % (loop, w, ", ".join(c) or "nothing (derived together with others, see REDUNDANT)")
                    for w, c in caught.items()))
    assert all(c for w, c in caught.items() if w not in grouped), [w for w, c in caught.items() if not c]
    for group in REDUNDANT.get(loop, []):
        assert not any(caught[w] for w in group), "a word of %s can be isolated after all: take it out of REDUNDANT" % (group,)
        whole = without(set(group))
        print("KEYWORD %s %-22s deleted together: caught by %s" % (loop, "/".join(group), ", ".join(whole)))
        assert whole, group
        for kept in group if len(group) > 2 else ():
            c = without(set(group) - {kept})
            print("KEYWORD %s %-22s alone of %s: the others' deletion is caught by %s" % (loop, kept, "/".join(group), ", ".join(c)))
            assert c, (group, kept)


def test_contents_and_host_staged_fields_are_live():
    """new contents at an old address, and what a call stages itself, must reach a REUSED graph: those rungs are MUST_REUSE and VALUE"""
    for loop in CL.KEYED:
        live = [r for r in CL.LADDERS[loop]["rungs"] if r.field.endswith("#") or r.field == "pad_id"]
        assert live, loop
        for r in live:
            assert (r.expect, r.kind) == (CL.MUST_REUSE, CL.VALUE), (loop, r.name)


def test_schedule_rules_mirror_gpt_hip():
    """att_phase, and the steps per graph, at the points the GPT ladders stand on (the device test asserts the same through plan_info and
    the capture counts)"""
    assert [CL.gpt_phase(kv, 14, None) for kv in (1, 16, 128, 129)] == [1, 1, 1, 2]             # 14 x 24 pairs < 512: the small regime
    assert [CL.gpt_phase(kv, 64, None) for kv in (1, 16, 256)] == [0, 0, 0]
    assert [CL.gpt_phase(kv, 14, (2, 4)) for kv in (1, 2, 3, 4, 5, 16)] == [0, 0, 1, 1, 2, 2]
    base = dict(CL.GPT_FUSED["base"])
    assert CL.gpt_group(base) == 4 and CL.gpt_group({**base, "steps": 12}) == 4 and CL.gpt_group({**base, "steps": 7}) == 1
    assert CL.gpt_group({**base, "steps": 16, "att_phases": (2, 4)}) == 1
    assert CL.gpt_slots({**base, "steps": 16, "att_phases": (2, 4)}, True) == {0, 1, 2, "B"}
