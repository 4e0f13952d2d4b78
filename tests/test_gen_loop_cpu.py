"""The generation loops of the decode engines (wmar_amd/csrc/gen_loop.h) on the CPU: tests/gen_loop_dump.cpp, built with the host compiler,
drives hooked_loop and grouped_loop with recording fakes; the exact sequence of drops, captures, replays and enqueues of every scenario is
checked here.  (@st: enqueued on the caller's stream, @cap: on the capture stream.)"""
import os
import subprocess

import pytest

from tests.conftest import REPO

OK, EINVAL, EHIP, ECALLBACK = 0, -1, -2, -6


@pytest.fixture(scope="module")
def scenarios(tmp_path_factory):
    """scenario name -> its output lines, through the dump program built once with the host compiler."""
    exe = str(tmp_path_factory.mktemp("gen_loop") / "gen_loop_dump")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", os.path.join(REPO, "tests", "gen_loop_dump.cpp"), "-o", exe])
    out, cur = {}, None
    for line in subprocess.check_output([exe]).decode().splitlines():
        if line.startswith("scenario "):
            cur = out.setdefault(line.split()[1], [])
        else:
            cur.append(line)
    return out


def call(rc, held, *events):
    return "call rc=%d held=%d: %s" % (rc, held, ", ".join(e for ev in events for e in ([ev] if isinstance(ev, str) else ev)))


def hooked_steps(a_slots, b_slot):
    """replay A, hook, replay B per step; an A slot of None: that step's A runs directly on the caller's stream."""
    out = []
    for n, s in enumerate(a_slots):
        out += ["A %d@st" % n if s is None else "replay %d@st" % s, "hook %d" % n, "replay %d@st" % b_slot]
    return out


CAPTURE_AB = ["drop", "capture 0", "A 0@cap", "capture 1", "B@cap"]


def test_hooked_one_slot_captures_once_per_key(scenarios):
    """First call: A then B captured, three steps, replayed.  Equal key: nothing dropped or captured.  One key word changed: again."""
    run = hooked_steps([0, 0, 0], 1) + ["replayed@st"]
    assert scenarios["hooked_one_slot"] == [call(OK, 1, CAPTURE_AB, run), call(OK, 1, run), call(OK, 1, CAPTURE_AB, run)]


def test_hooked_captures_only_the_slots_its_steps_need(scenarios):
    """slot_of = 0, 0, 1 of three A slots: slots 0, 1 and B (slot 3) are captured, each A slot with the first step that maps to it.  A
    later call under the same key whose fourth step needs slot 2 drops everything and captures 0, 1, 2 and B."""
    run3 = hooked_steps([0, 0, 1], 3) + ["replayed@st"]
    run4 = hooked_steps([0, 0, 1, 2], 3) + ["replayed@st"]
    assert scenarios["hooked_three_slots"] == [
        call(OK, 1, "drop", "capture 0", "A 0@cap", "capture 1", "A 2@cap", "capture 3", "B@cap", run3),
        call(OK, 1, run3),
        call(OK, 1, "drop", "capture 0", "A 0@cap", "capture 1", "A 2@cap", "capture 2", "A 3@cap", "capture 3", "B@cap", run4),
    ]


def test_hooked_negative_slot_runs_that_step_directly(scenarios):
    """slot_of(0) < 0 (Chameleon: the first image token comes from the prefill logits): A 0 runs on the caller's stream, slot 0 is captured
    with step 1.  A one-step call under the same key needs only B, which is there."""
    assert scenarios["hooked_eager_first_step"] == [
        call(OK, 1, "drop", "capture 0", "A 1@cap", "capture 1", "B@cap", hooked_steps([None, 0, 0], 1), "replayed@st"),
        call(OK, 1, hooked_steps([None], 1), "replayed@st"),
    ]


def test_hook_failure_stops_the_loop_and_keeps_the_graphs(scenarios):
    """The hook fails at step 1: no B behind it, replayed all the same, the hook's status returned; graphs and key are kept."""
    assert scenarios["hook_fails"] == [
        call(ECALLBACK, 1, CAPTURE_AB, hooked_steps([0], 1), "replay 0@st", "hook 1", "replayed@st"),
        call(OK, 1, hooked_steps([0, 0, 0], 1), "replayed@st"),
    ]


def test_failed_capture_leaves_no_key_behind(scenarios):
    """The capture of B fails (it drops every slot, as GraphSlots::capture does): its status is returned, nothing is replayed, the held
    key is reset; the next call with that key captures again."""
    run = hooked_steps([0, 0], 1) + ["replayed@st"]
    assert scenarios["capture_of_b_fails"] == [call(OK, 1, CAPTURE_AB, run), call(EHIP, 0, CAPTURE_AB, "drop"), call(OK, 1, CAPTURE_AB, run)]


def test_eager_loops_touch_no_graph(scenarios):
    """use_graph off: no drop, capture, replay or replayed; A / hook / B and the fused steps in order on the caller's stream, the held key
    untouched; a failing hook ends the loop behind it."""
    assert scenarios["eager"] == [
        call(OK, 0, "A 0@st", "hook 0", "B@st", "A 1@st", "hook 1", "B@st"),
        call(ECALLBACK, 0, "A 0@st", "hook 0"),
        call(OK, 0, "step 0@st", "step 1@st", "step 2@st"),
    ]


def test_grouped_keyed(scenarios):
    """8 steps in groups of 4: one capture of four steps, two replays, replayed; a repeat captures nothing.  6 steps, gs = 1, slots
    0 0 0 1 1 1: two captures (steps 0 and 3), six replays in slot order; a repeat captures nothing; the same key with steps that reach a
    slot without a graph captures all three."""
    assert scenarios["grouped_keyed"] == [
        call(OK, 1, "drop", "capture 0", ["step %d@cap" % n for n in range(4)], ["replay 0@st"] * 2, "replayed@st"),
        call(OK, 1, ["replay 0@st"] * 2, "replayed@st"),
        call(OK, 1, "drop", "capture 0", "step 0@cap", "capture 1", "step 3@cap", ["replay 0@st"] * 3, ["replay 1@st"] * 3, "replayed@st"),
        call(OK, 1, ["replay 0@st"] * 3, ["replay 1@st"] * 3, "replayed@st"),
        call(OK, 1, "drop", "capture 0", "step 0@cap", "capture 1", "step 2@cap", "capture 2", "step 4@cap", ["replay 0@st"] * 2,
             ["replay 1@st"] * 2, ["replay 2@st"] * 2, "replayed@st"),
    ]


def test_grouped_keyless_captures_on_every_call(scenarios):
    """7 steps, lead 3, groups of 4, no held key: three steps directly, then drop, one capture of steps 3..6, one replay, replayed -- and
    the same again on the second call.  Only lead steps: no graph is touched.  Steps that do not fill their groups are refused."""
    full = call(OK, 0, ["step %d@st" % n for n in range(3)], "drop", "capture 0", ["step %d@cap" % n for n in range(3, 7)], "replay 0@st",
                "replayed@st")
    assert scenarios["grouped_keyless"] == [
        full, full, call(OK, 0, ["step %d@st" % n for n in range(3)]),
        call(EINVAL, 0, "step 0@st", "step 1@st", "error: generation loop: 5 steps do not fill groups of 4"),
    ]


def test_graph_key(scenarios):
    """Equal sequences are equal; a word or the length makes a difference; floats compare by bits (NaN == NaN, -0.0 != 0.0); a default key
    equals nothing, itself included; a key filled to capacity works, one word more is an overflow that equals nothing and that both loops
    refuse before they touch a graph."""
    assert scenarios["graph_key"] == [
        "equal_sequences 1", "other_word 0", "other_length 0", "nan_equals_nan 1", "neg_zero_equals_zero 0", "f64_by_bits 0 1",
        "default_equals_built 0 0", "default_equals_default 0", "full_equals_full 1 overflow 0 1", "overflowed_equals 0 0",
        call(EINVAL, 0, "error: graph key: more than 16 words"), call(EINVAL, 0, "error: graph key: more than 16 words"),
    ]
