// The generation loop of the decode engines (gpt.hip, rar.hip, cham.hip): when captured graphs are reused, when they are captured
// again, and in which order a step's pieces are enqueued.  No HIP here: the loops are templates over the slots type (the engines
// pass GraphSlots<N>, decoder_host.h) and the stream type, so that tests/gen_loop_dump.cpp drives them with a recording fake.
//
// A slots type has: n_slots, has(slot), drop(), capture(slot, enqueue(capture_stream)), replay(slot, stream), replayed(stream).
// A capture that fails has dropped every slot (GraphSlots::capture does).
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/wmar_hip.h"

namespace wmar {

void set_error(const char* fmt, ...);      // the library's error text (keytable.cpp)

// Everything the launches of a captured graph depend on -- batch, lengths, pointers, sampling scalars -- as 64-bit words.  A graph
// is replayed only under the key it was captured with.  Floats go in by bit pattern: NaN equals itself, -0.0f differs from 0.0f.
struct GraphKey {
    static constexpr int CAP = 16;
    uint64_t w[CAP] = {};
    int n = 0;                   // words appended; none: the key of "no graph", equal to no key (itself included)
    bool overflow = false;       // an append beyond CAP: the loops refuse such a key
    GraphKey& u64(uint64_t v) { if (n < CAP) w[n++] = v; else overflow = true; return *this; }
    GraphKey& i32(int32_t v) { return u64((uint64_t)(int64_t)v); }
    GraphKey& ptr(const void* p) { return u64((uint64_t)(uintptr_t)p); }
    GraphKey& f32(float v) { uint32_t b; memcpy(&b, &v, 4); return u64(b); }
    GraphKey& f64(double v) { uint64_t b; memcpy(&b, &v, 8); return u64(b); }
    bool operator==(const GraphKey& o) const { return n > 0 && n == o.n && !overflow && !o.overflow && memcmp(w, o.w, (size_t)n * 8) == 0; }
    bool operator!=(const GraphKey& o) const { return !(*this == o); }
};

// Make every slot the steps first, first + gs, .. < n_steps map to (slot_of(n) >= 0), and slot_b when >= 0, hold a graph captured
// under `want`.  They are kept when `held` equals `want` and each of them has a graph; otherwise ALL slots are dropped, the held
// key is reset, the needed slots are captured in slot order -- slot s as one_step(cap, n) .. one_step(cap, n + gs - 1) for the first
// n that maps to it, slot_b as step_b(cap) -- and the key is stored last, so that a failed capture leaves no key behind.
// held == nullptr: no reuse, drop and capture on every call.
template <typename Slots, typename SlotOf, typename Step, typename StepB>
int ensure_graphs(Slots& slots, GraphKey* held, const GraphKey& want, int first, int n_steps, int gs, int slot_b, SlotOf&& slot_of,
                  Step&& one_step, StepB&& step_b) {
    if (want.overflow) { set_error("graph key: more than %d words", GraphKey::CAP); return WMAR_EINVAL; }
    int first_n[Slots::n_slots];
    for (int s = 0; s < Slots::n_slots; ++s) first_n[s] = -1;
    for (int n = n_steps - gs; n >= first; n -= gs) {
        const int s = slot_of(n);
        if (s >= Slots::n_slots || s == slot_b) { set_error("generation loop: step %d maps to slot %d", n, s); return WMAR_EINVAL; }
        if (s >= 0) first_n[s] = n;
    }
    bool have = held && *held == want && (slot_b < 0 || slots.has(slot_b));
    for (int s = 0; s < Slots::n_slots; ++s) have = have && (first_n[s] < 0 || slots.has(s));
    if (have) return WMAR_OK;
    slots.drop();
    if (held) *held = GraphKey();
    for (int s = 0; s < Slots::n_slots; ++s) {
        if (first_n[s] < 0) continue;
        const int rc = slots.capture(s, [&](auto cap) {
            int r = WMAR_OK;
            for (int k = 0; k < gs && r == WMAR_OK; ++k) r = one_step(cap, first_n[s] + k);
            return r;
        });
        if (rc) return rc;
    }
    if (slot_b >= 0) { if (int rc = slots.capture(slot_b, step_b)) return rc; }
    if (held) *held = want;
    return WMAR_OK;
}

// A step cut in two around a host callback: step_a(stream, n), hook(n), step_b(stream), n = 0 .. n_steps - 1, stopped at the first
// status that is not WMAR_OK.  With use_graph, step n's first half is a replay of slot slot_of(n) (negative: step_a runs directly
// on `stream` for this step) and the second half a replay of the LAST slot; the graphs live under `held` (ensure_graphs).
// replayed() follows the last step also when the hook failed: the replays enqueued up to there are still running.
template <typename Slots, typename Stream, typename SlotOf, typename StepA, typename Hook, typename StepB>
int hooked_loop(Slots& slots, GraphKey& held, const GraphKey& want, bool use_graph, int n_steps, SlotOf&& slot_of, StepA&& step_a,
                Hook&& hook, StepB&& step_b, Stream stream) {
    constexpr int SLOT_B = Slots::n_slots - 1;
    if (use_graph) {
        if (int rc = ensure_graphs(slots, &held, want, 0, n_steps, 1, SLOT_B, slot_of, step_a, step_b)) return rc;
    }
    int rc = WMAR_OK;
    for (int n = 0; n < n_steps && rc == WMAR_OK; ++n) {
        const int s = use_graph ? slot_of(n) : -1;
        rc = s >= 0 ? slots.replay(s, stream) : step_a(stream, n);
        if (rc == WMAR_OK) rc = hook(n);
        if (rc == WMAR_OK) rc = use_graph ? slots.replay(SLOT_B, stream) : step_b(stream);
    }
    if (use_graph) { const int r = slots.replayed(stream); if (rc == WMAR_OK) rc = r; }
    return rc;
}

// The fused step one_step(stream, n), n = 0 .. n_steps - 1.  With use_graph the first `lead` steps run directly on `stream` and
// the others in groups of gs, a group being ONE replay of slot slot_of(n) of its first step n (>= 0); the caller guarantees
// (n_steps - lead) % gs == 0 and passes gs == 1 when the steps map to more than one slot.  The graphs live under `held`, or are
// captured by every call when it is null (ensure_graphs).  replayed() follows the last replay.
template <typename Slots, typename Stream, typename SlotOf, typename Step>
int grouped_loop(Slots& slots, GraphKey* held, const GraphKey& want, bool use_graph, int n_steps, int lead, int gs, SlotOf&& slot_of,
                 Step&& one_step, Stream stream) {
    if (!use_graph) lead = n_steps;
    int rc = WMAR_OK;
    for (int n = 0; n < lead && rc == WMAR_OK; ++n) rc = one_step(stream, n);
    if (rc != WMAR_OK || lead >= n_steps) return rc;
    if (gs < 1 || (n_steps - lead) % gs != 0) { set_error("generation loop: %d steps do not fill groups of %d", n_steps - lead, gs); return WMAR_EINVAL; }
    if ((rc = ensure_graphs(slots, held, want, lead, n_steps, gs, -1, slot_of, one_step, [](Stream) { return WMAR_OK; }))) return rc;
    for (int n = lead; n < n_steps && rc == WMAR_OK; n += gs) rc = slots.replay(slot_of(n), stream);
    const int r = slots.replayed(stream);
    return rc != WMAR_OK ? rc : r;
}

}  // namespace wmar
