"""Call ladders of the generation loops that keep captured graphs from one call to the next -- the data of
tests/test_call_ladders_cpu.py (a host model of keyed reuse) and tests/test_gpu_call_state.py (the same ladders on the device).

A ladder is a base call and a list of rungs.  A call is a dict of FIELDS; a rung names ONE field and its new value, every other field
keeps the value of the call before it (the ladder is a chain, not a star).  Field names:

    name        a scalar or a switch of the call (B, steps, temperature, wm, timing, ...)
    name@       WHERE a buffer lives: an index into the test's pool of allocations (None: a null pointer)
    name#       WHAT a buffer holds: the seed / variant its contents are made from

What a rung expects of the graphs:  MUST_REUSE -- the call replays what the call before it left, the engine's capture counter stays;
MAY_CAPTURE -- the call has to capture (the counter moves).  The device test holds the counter to "moved if and only if MAY_CAPTURE".

What a rung expects of the RESULT (kind):
    VALUE     the result depends on the field: the eager twin's output differs from its output for the call before (asserted: a rung
              whose outputs cannot differ would pass with a stale graph)
    ADDRESS   only where a buffer lives (or how it is laid out) changes: outputs are prefilled with -1, the new buffer is written, the
              old one is not touched; the values written equal the call before
    NEUTRAL   by contract no effect on the result (an exact repeat, the timing switch, the row compaction of the Chameleon sampler)
"""
from collections import namedtuple

MUST_REUSE, MAY_CAPTURE = "must_reuse", "may_capture"
VALUE, ADDRESS, NEUTRAL = "value", "address", "neutral"

Rung = namedtuple("Rung", "name field value expect kind")


def R(name, field, value, expect, kind=VALUE):
    return Rung(name, field, value, expect, kind)


def nextafter_up(x: float) -> float:
    """the next double above x (x > 0)"""
    import struct
    return struct.unpack("<d", struct.pack("<q", struct.unpack("<q", struct.pack("<d", x))[0] + 1))[0]


TOP_P = 0.8
# The synthetic heads give logits with a standard deviation of about 7: at temperature 1 nearly every token is the row's largest logit
# and top-k, a watermark bias or a changed hook would move nothing.  At 3 a Gaussian row of that width loses a token in eight to
# top_p 0.8, one in two to top_k 50, one in seven to a delta of 2 -- over the 100 (GPT), 32 (RAR) and 36 (Chameleon) tokens of a call.
BASE_T = 3.0
LINEAR, SPATIAL, FIXED = 1, 2, 0            # WMAR_SEED_* (include/wmar_hip.h)
N_ROWS_FULL, N_ROWS_CUT = 2 * (16384 - 1) + 1, 9000     # key table rows for context sums of two ids; a cut that drops the bias of sums >= 9000

_SAMPLING = [
    R("temperature", "temperature", 4.2, MAY_CAPTURE),
    R("top_k_on", "top_k", 50, MAY_CAPTURE), R("top_k_off", "top_k", 0, MAY_CAPTURE), R("top_k_other", "top_k", 100, MAY_CAPTURE),
    R("top_p_on", "top_p", TOP_P, MAY_CAPTURE), R("top_p_off", "top_p", -1.0, MAY_CAPTURE),
    R("top_p_next_double", "top_p", nextafter_up(TOP_P), MAY_CAPTURE),
]
# 13..32-row plan -> small-batch plan (<= 12 rows) -> back above it
_GPT_SHAPE = [
    R("steps_12", "steps", 12, MAY_CAPTURE), R("steps_7", "steps", 7, MAY_CAPTURE),          # groups of 4 steps, then of 1
    R("B_13_to_12", "B", 12, MAY_CAPTURE), R("B_12_to_14", "B", 14, MAY_CAPTURE),
]

GPT_FUSED = dict(
    keyed=True,
    base={"B": 13, "steps": 8, "temperature": BASE_T, "top_k": 0, "top_p": -1.0,
          "wm": True, "delta": 2.0, "table@": 0, "table#": 0, "n_rows": N_ROWS_FULL, "seed_strategy": LINEAR, "context_size": 1,
          "spatial_dim": 2, "q@": 0, "q#": 0, "cond#": 0, "out@": 0, "trace@": 0, "att_phases": None, "timing": 0},
    rungs=[R("repeat", "B", 13, MUST_REUSE, NEUTRAL)] + _SAMPLING + [
        R("delta_0", "delta", 0.0, MAY_CAPTURE), R("delta_other", "delta", 3.5, MAY_CAPTURE),
        R("wm_null", "wm", False, MAY_CAPTURE), R("wm_set", "wm", True, MAY_CAPTURE),
        R("table_other_address", "table@", 1, MAY_CAPTURE, ADDRESS),
        R("table_rebuilt_in_place", "table#", 1, MUST_REUSE),                 # same address, another salt: the tokens follow the contents
        R("n_rows_cut", "n_rows", N_ROWS_CUT, MAY_CAPTURE), R("n_rows_full", "n_rows", N_ROWS_FULL, MAY_CAPTURE),
        R("context_2", "context_size", 2, MAY_CAPTURE), R("context_1", "context_size", 1, MAY_CAPTURE),
        R("spatial", "seed_strategy", SPATIAL, MAY_CAPTURE), R("spatial_dim", "spatial_dim", 4, MAY_CAPTURE),
        R("fixed", "seed_strategy", FIXED, MAY_CAPTURE),
    ] + _GPT_SHAPE + [
        R("q_other_address", "q@", 1, MAY_CAPTURE, ADDRESS), R("out_other_address", "out@", 1, MAY_CAPTURE, ADDRESS),
        R("trace_null", "trace@", None, MAY_CAPTURE, ADDRESS), R("trace_other_address", "trace@", 1, MAY_CAPTURE, ADDRESS),
        R("q_new_contents", "q#", 1, MUST_REUSE), R("cond_new_contents", "cond#", 1, MUST_REUSE),
        R("steps_40", "steps", 40, MAY_CAPTURE),
        # 40 steps: a wave of the decode attention streams the cache in chunks of 8 rows, so up to 16 cached rows every schedule does the
        # same arithmetic and the rung would move no bit; at 40 rows two waves and four split the chunks differently.  (2, 4): three
        # phases, three slots; wmar_gpt_set_attention_phases drops the fused graphs whenever the schedule changes
        R("phases_2_4", "att_phases", (2, 4), MAY_CAPTURE), R("phases_auto", "att_phases", None, MAY_CAPTURE),
        R("timing_on", "timing", 1, MUST_REUSE, NEUTRAL), R("timing_off", "timing", 0, MUST_REUSE, NEUTRAL),
    ])

GPT_HOOKED = dict(
    keyed=True,
    base={"B": 13, "steps": 8, "temperature": BASE_T, "top_k": 0, "top_p": -1.0, "q@": 0, "q#": 0, "cond#": 0, "out@": 0,
          "hook_logits@": 0, "hook_past@": 0, "past_stride": 41, "att_phases": None},
    rungs=[R("repeat", "B", 13, MUST_REUSE, NEUTRAL)] + _SAMPLING + _GPT_SHAPE + [
        R("q_other_address", "q@", 1, MAY_CAPTURE, ADDRESS), R("out_other_address", "out@", 1, MAY_CAPTURE, ADDRESS),
        R("hook_logits_other_address", "hook_logits@", 1, MAY_CAPTURE, ADDRESS),
        R("hook_past_other_address", "hook_past@", 1, MAY_CAPTURE, ADDRESS),
        R("past_stride", "past_stride", 44, MAY_CAPTURE, ADDRESS),
        R("q_new_contents", "q#", 1, MUST_REUSE), R("cond_new_contents", "cond#", 1, MUST_REUSE),
        R("steps_40", "steps", 40, MAY_CAPTURE),
        # 14 rows, automatic schedule: every step is phase 1.  (2, 4): phases 0, 1, 2 -- slot 0 has no graph: everything is captured.
        # Back to automatic: phase 1 only, whose slot (and the sampler's) the call before left, under an equal key: a reuse although
        # wmar_gpt_set_attention_phases does not drop the hooked graphs -- a slot's graph depends on the phase alone.
        R("phases_2_4", "att_phases", (2, 4), MAY_CAPTURE), R("phases_auto", "att_phases", None, MUST_REUSE),
    ])

# rows: guidance and batch in one word -- g2 (guided, B = 2) and u4 (unguided, B = 4) both run M = 4 rows
RAR_HOOKED = dict(
    keyed=True,
    base={"rows": "g2", "temperature": BASE_T, "q@": 0, "q#": 0, "class#": 0, "cfg_scales#": 0, "out@": 0, "hook_logits@": 0,
          "hook_past@": 0, "past_stride": 16},
    rungs=[
        R("repeat", "rows", "g2", MUST_REUSE, NEUTRAL), R("temperature", "temperature", 4.2, MAY_CAPTURE),
        R("cfg_scales_new_contents", "cfg_scales#", 1, MUST_REUSE),
        R("guided_2_to_unguided_4", "rows", "u4", MAY_CAPTURE), R("unguided_3", "rows", "u3", MAY_CAPTURE),
        R("guided_3", "rows", "g3", MAY_CAPTURE),
        R("q_other_address", "q@", 1, MAY_CAPTURE, ADDRESS), R("out_other_address", "out@", 1, MAY_CAPTURE, ADDRESS),
        R("hook_logits_other_address", "hook_logits@", 1, MAY_CAPTURE, ADDRESS),
        R("hook_past_other_address", "hook_past@", 1, MAY_CAPTURE, ADDRESS),
        R("past_stride", "past_stride", 19, MAY_CAPTURE, ADDRESS),
        R("q_new_contents", "q#", 1, MUST_REUSE), R("class_ids_new_contents", "class#", 1, MUST_REUSE),
    ])

CHAM_HOOKED = dict(
    keyed=True,
    base={"B": 3, "n_tokens": 12, "temperature": BASE_T, "top_p": -1.0, "g_text": 3.0, "g_image": 1.2, "pad_id": 1, "prompts#": 0,
          "compaction": False, "allow@": 0, "allow#": 0, "q@": 0, "q#": 0, "out@": 0, "hook_logits@": 0, "hook_past@": 0,
          "past_stride": 24},
    rungs=[
        R("repeat", "B", 3, MUST_REUSE, NEUTRAL), R("temperature", "temperature", 4.2, MAY_CAPTURE),
        R("top_p_on", "top_p", TOP_P, MAY_CAPTURE), R("top_p_off", "top_p", -1.0, MAY_CAPTURE),
        R("top_p_next_double", "top_p", nextafter_up(TOP_P), MAY_CAPTURE),
        R("guidance_text", "g_text", 2.0, MAY_CAPTURE), R("guidance_image", "g_image", 1.7, MAY_CAPTURE),
        R("n_tokens", "n_tokens", 16, MAY_CAPTURE),
        # other lengths in the same host arrays' places: maxlen (5 -> 7) reaches the launches only through device counters
        R("prompt_lengths", "prompts#", 1, MUST_REUSE), R("pad_id", "pad_id", 3, MUST_REUSE),
        R("compaction_on", "compaction", True, MAY_CAPTURE, NEUTRAL), R("compaction_off", "compaction", False, MAY_CAPTURE, NEUTRAL),
        R("allow_new_contents", "allow#", 1, MUST_REUSE), R("allow_other_address", "allow@", 1, MAY_CAPTURE, ADDRESS),
        R("B_3_to_2", "B", 2, MAY_CAPTURE),
        R("q_other_address", "q@", 1, MAY_CAPTURE, ADDRESS), R("out_other_address", "out@", 1, MAY_CAPTURE, ADDRESS),
        R("hook_logits_other_address", "hook_logits@", 1, MAY_CAPTURE, ADDRESS),
        R("hook_past_other_address", "hook_past@", 1, MAY_CAPTURE, ADDRESS),
        R("past_stride", "past_stride", 27, MAY_CAPTURE, ADDRESS),
        R("q_new_contents", "q#", 1, MUST_REUSE),
    ])

# The keyless loops (wmar_rar_generate, _gumbel, _gumbel_ctx, wmar_cham_generate_image) capture on every call: nothing to reuse, no
# rungs.  Their base calls take part in the history lists of tests/test_gpu_call_state.py only.
RAR_FUSED = dict(keyed=False, base={"rows": "g4", "temperature": 1.0, "wm": False}, rungs=[])
RAR_GUMBEL = dict(keyed=False, base={"rows": "g4", "temperature": 1.0, "top_p": 0.0, "top_k": 0}, rungs=[])
RAR_GUMBEL_CTX = dict(keyed=False, base={"rows": "g4", "temperature": 1.0, "top_p": 0.0, "top_k": 0, "ngram": 2}, rungs=[])
CHAM_FUSED = dict(keyed=False, base={"B": 3, "n_tokens": 8, "temperature": 0.9, "top_p": -1.0, "compaction": False}, rungs=[])

LADDERS = {"gpt_fused": GPT_FUSED, "gpt_hooked": GPT_HOOKED, "rar_hooked": RAR_HOOKED, "cham_hooked": CHAM_HOOKED,
           "rar_fused": RAR_FUSED, "rar_gumbel": RAR_GUMBEL, "rar_gumbel_ctx": RAR_GUMBEL_CTX, "cham_fused": CHAM_FUSED}
KEYED = [k for k, v in LADDERS.items() if v["keyed"]]


def rar_rows(word):
    """rows word -> (guided, B)"""
    return word[0] == "g", int(word[1:])


def calls(loop):
    """[(rung or None, call)]: the base call, then every rung's call with the rung's field replaced in the call before it"""
    lad = LADDERS[loop]
    cur = dict(lad["base"])
    out = [(None, dict(cur))]
    for r in lad["rungs"]:
        assert r.field in cur, (loop, r.name, r.field)
        cur[r.field] = r.value
        out.append((r, dict(cur)))
    return out


# ------------------------------------------------------------------------------------------------ the engines' rules, on the host
GPT_HEADS = 24                  # the engine of the GPT ladders (production width)
GRAPH_STEPS_DEFAULT = 4         # gpt.hip


def gpt_phase(kv, B, att_phases, heads=GPT_HEADS):
    """wmar_gpt::att_phase (gpt.hip): the attention phase of the step that attends to kv cached rows"""
    if att_phases is None:
        return (1 if kv <= 128 else 2) if B * heads < 512 else 0
    return 0 if kv <= att_phases[0] else (1 if kv <= att_phases[1] else 2)


def gpt_slots(call, hooked):
    """the graph slots a GPT call replays: one per attention phase its steps pass through; hooked: and the sampler's"""
    s = {gpt_phase(n + 1, call["B"], call["att_phases"]) for n in range(call["steps"])}
    return s | {"B"} if hooked else s


def gpt_group(call):
    """steps per captured graph of the fused loop"""
    return GRAPH_STEPS_DEFAULT if len(gpt_slots(call, False)) == 1 and call["steps"] % GRAPH_STEPS_DEFAULT == 0 else 1
