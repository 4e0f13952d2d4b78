// Drives the generation loops (wmar_amd/csrc/gen_loop.h) with recording fakes and prints what they did, for
// tests/test_gen_loop_cpu.py.  Host-only.  Output: "scenario <name>", then per call "call rc=<status> held=<0|1>: <log>", the log being
// the comma-separated events drop | capture s | replay s | replayed | A n | hook n | B | step n, each enqueue with its stream (@st: the
// caller's, @cap: the capture stream); held = the held key equals the call's key afterwards.
#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <string>

#include "../wmar_amd/csrc/gen_loop.h"

static std::string g_log;
static void ev(const std::string& e) { g_log += (g_log.empty() ? "" : ", ") + e; }

namespace wmar {
void set_error(const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    ev(std::string("error: ") + buf);
}
}  // namespace wmar

using wmar::GraphKey;

enum Stream { ST = 0, CAP = 1 };
static std::string at(Stream s) { return s == CAP ? "@cap" : "@st"; }
static std::string num(int v) { return std::to_string(v); }

template <int N>
struct FakeSlots {
    static constexpr int n_slots = N;
    bool exec[N] = {};
    int fail_capture = -1;       // the next capture of this slot fails (once), as a failed instantiation would
    bool has(int s) const { return exec[s]; }
    void drop() { ev("drop"); for (bool& e : exec) e = false; }
    template <typename F>
    int capture(int s, F&& enqueue) {
        ev("capture " + num(s));
        int rc = enqueue(CAP);
        if (rc == WMAR_OK && s == fail_capture) { fail_capture = -1; rc = WMAR_EHIP; }
        if (rc != WMAR_OK) drop(); else exec[s] = true;
        return rc;
    }
    int replay(int s, Stream st) { ev("replay " + num(s) + at(st)); return exec[s] ? WMAR_OK : WMAR_EHIP; }
    int replayed(Stream st) { ev("replayed" + at(st)); return WMAR_OK; }
};

static int step_a(Stream s, int n) { ev("A " + num(n) + at(s)); return WMAR_OK; }
static int step_b(Stream s) { ev("B" + at(s)); return WMAR_OK; }
static int one_step(Stream s, int n) { ev("step " + num(n) + at(s)); return WMAR_OK; }
static int g_hook_fails_at = -1;
static int hook(int n) { ev("hook " + num(n)); return n == g_hook_fails_at ? WMAR_ECALLBACK : WMAR_OK; }

static void report(int rc, const GraphKey* held, const GraphKey& want) {
    printf("call rc=%d held=%d: %s\n", rc, held && *held == want ? 1 : 0, g_log.c_str());
    g_log.clear();
}

template <int N, typename SlotOf>
static void hooked(FakeSlots<N>& sl, GraphKey& held, const GraphKey& want, bool graph, int n, SlotOf slot_of) {
    report(wmar::hooked_loop(sl, held, want, graph, n, slot_of, step_a, hook, step_b, ST), &held, want);
}
template <int N, typename SlotOf>
static void grouped(FakeSlots<N>& sl, GraphKey* held, const GraphKey& want, bool graph, int n, int lead, int gs, SlotOf slot_of) {
    report(wmar::grouped_loop(sl, held, want, graph, n, lead, gs, slot_of, one_step, ST), held, want);
}

int main() {
    const GraphKey k1 = GraphKey().u64(64).ptr(&g_log).f32(1.0f).f64(0.92), k2 = GraphKey().u64(64).ptr(&g_log).f32(1.0f).f64(0.95);
    auto slot0 = [](int) { return 0; };
    {
        printf("scenario hooked_one_slot\n");
        FakeSlots<2> sl; GraphKey held;
        hooked(sl, held, k1, true, 3, slot0);
        hooked(sl, held, k1, true, 3, slot0);
        hooked(sl, held, k2, true, 3, slot0);
    }
    {
        printf("scenario hooked_three_slots\n");
        FakeSlots<4> sl; GraphKey held;
        hooked(sl, held, k1, true, 3, [](int n) { return n < 2 ? 0 : 1; });
        hooked(sl, held, k1, true, 3, [](int n) { return n < 2 ? 0 : 1; });
        hooked(sl, held, k1, true, 4, [](int n) { return n < 2 ? 0 : n - 1; });
    }
    {
        printf("scenario hooked_eager_first_step\n");
        FakeSlots<2> sl; GraphKey held;
        hooked(sl, held, k1, true, 3, [](int n) { return n > 0 ? 0 : -1; });
        hooked(sl, held, k1, true, 1, [](int n) { return n > 0 ? 0 : -1; });
    }
    {
        printf("scenario hook_fails\n");
        FakeSlots<2> sl; GraphKey held;
        g_hook_fails_at = 1;
        hooked(sl, held, k1, true, 3, slot0);
        g_hook_fails_at = -1;
        hooked(sl, held, k1, true, 3, slot0);
    }
    {
        printf("scenario capture_of_b_fails\n");
        FakeSlots<2> sl; GraphKey held;
        hooked(sl, held, k1, true, 2, slot0);
        sl.fail_capture = 1;
        hooked(sl, held, k2, true, 2, slot0);
        hooked(sl, held, k2, true, 2, slot0);
    }
    {
        printf("scenario eager\n");
        FakeSlots<2> sl; GraphKey held;
        hooked(sl, held, k1, false, 2, slot0);
        g_hook_fails_at = 0;
        hooked(sl, held, k1, false, 2, slot0);
        g_hook_fails_at = -1;
        grouped(sl, &held, k1, false, 3, 1, 2, slot0);
    }
    {
        printf("scenario grouped_keyed\n");
        FakeSlots<3> sl; GraphKey held;
        grouped(sl, &held, k1, true, 8, 0, 4, slot0);
        grouped(sl, &held, k1, true, 8, 0, 4, slot0);
        grouped(sl, &held, k2, true, 6, 0, 1, [](int n) { return n / 3; });
        grouped(sl, &held, k2, true, 6, 0, 1, [](int n) { return n / 3; });
        grouped(sl, &held, k2, true, 6, 0, 1, [](int n) { return n / 2; });
    }
    {
        printf("scenario grouped_keyless\n");
        FakeSlots<1> sl;
        grouped(sl, nullptr, GraphKey(), true, 7, 3, 4, slot0);
        grouped(sl, nullptr, GraphKey(), true, 7, 3, 4, slot0);
        grouped(sl, nullptr, GraphKey(), true, 3, 3, 4, slot0);
        grouped(sl, nullptr, GraphKey(), true, 7, 2, 4, slot0);
    }
    {
        printf("scenario graph_key\n");
        const float nan = std::nanf(""), inf = INFINITY;
        GraphKey full;
        for (int i = 0; i < GraphKey::CAP; ++i) full.u64((uint64_t)i);
        GraphKey over = full;
        over.i32(1);
        printf("equal_sequences %d\n", (int)(GraphKey().u64(1).i32(-2).ptr(&full) == GraphKey().u64(1).i32(-2).ptr(&full)));
        printf("other_word %d\n", (int)(GraphKey().u64(1).i32(-2) == GraphKey().u64(1).i32(2)));
        printf("other_length %d\n", (int)(GraphKey().u64(1) == GraphKey().u64(1).u64(0)));
        printf("nan_equals_nan %d\n", (int)(GraphKey().f32(nan) == GraphKey().f32(nan)));
        printf("neg_zero_equals_zero %d\n", (int)(GraphKey().f32(-0.0f) == GraphKey().f32(0.0f)));
        printf("f64_by_bits %d %d\n", (int)(GraphKey().f64(-0.0) == GraphKey().f64(0.0)), (int)(GraphKey().f64(inf) == GraphKey().f64(inf)));
        printf("default_equals_built %d %d\n", (int)(GraphKey() == GraphKey().u64(0)), (int)(GraphKey().u64(0) == GraphKey()));
        printf("default_equals_default %d\n", (int)(GraphKey() == GraphKey()));
        printf("full_equals_full %d overflow %d %d\n", (int)(full == full), (int)full.overflow, (int)over.overflow);
        printf("overflowed_equals %d %d\n", (int)(over == over), (int)(over == full));
        FakeSlots<2> sl; GraphKey held;
        hooked(sl, held, over, true, 2, slot0);
        grouped(sl, &held, over, true, 4, 0, 4, slot0);
    }
    return 0;
}
