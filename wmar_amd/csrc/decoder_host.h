// Host-side scaffold shared by the decode engines (gpt.hip, rar.hip, cham.hip): weight packing and GEMM dispatch, and the
// mechanisms every engine drives its kernels with -- captured-graph lifetime (GraphSlots), the "whole grid resident" check, the
// block -> XCD grouping probe, the re-run behind a failed in-launch barrier and the sampler + counters tail of a generation step.
// The generation loop itself -- graph key, capture rule, hooked and grouped step order -- is in gen_loop.h, free of HIP so that it
// is tested on the CPU; the sampler arguments every loop fills are loop_samp_args (sampler.h).  (The allocation list and the
// checkpoint lookup are in common.h: vqgan.hip uses them without these kernels.)  The test-only stage access the engines share
// is in probe_host.h.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "decoder_kernels.h"
#include "gen_loop.h"

namespace wmar {

inline int mt_for(int64_t B) { return B <= 32 ? 1 : (B <= 64 ? 2 : 4); }

inline int pack(const float* W, float4* Wp, int N, int K, int nt_off, hipStream_t st,
         const float* gamma = nullptr) {
    long long total = (long long)(N / 32) * (K / 8) * 64;
    hipLaunchKernelGGL(k_pack_linear, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, W, Wp, N, K, nt_off, K / 8,
                       gamma);
    return launch_status("k_pack_linear");
}

// W[N][K] (columns scaled by gamma when given) -> Wq in k_pack_bx order, N / 32 column tiles from tile `tile_off` on
inline int pack_bx(const float* W, const float* gamma, float4* Wq, int N, int K, int tile_off, hipStream_t st) {
    const long long total = (long long)(N / 32) * (K / 16) * 128;
    hipLaunchKernelGGL(k_pack_bx, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, W, gamma, Wq, N, K, tile_off);
    return launch_status("k_pack_bx");
}

// dst[0..N) = bias + W beta
inline int fold_bias(const float* W, const float* bias, const float* beta, float* dst, int N, int K, hipStream_t st) {
    hipLaunchKernelGGL(k_fold_bias, dim3((unsigned)N), dim3(64), 0, st, W, bias, beta, dst, K);
    return launch_status("k_fold_bias");
}

template <typename Engine>
int copy_vec(Engine* g, float** dst, const float* src, size_t n, hipStream_t st) {
    if (int rc = g->mem.alloc(dst, n)) return rc;
    WMAR_HIP_CHECK(hipMemcpyAsync(*dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return WMAR_OK;
}

template <int MTW, int NW, int EPI, bool LN, int ABL = 0, int U = GEMM_STAGE, bool ROT = true, int NTW = 1>
int launch_gemm(const GemmArgs& a, hipStream_t st) {
    const int grid = NTW > 1 ? (a.NT / NTW) * (a.MT / MTW) : a.NT * (a.MT / MTW) * a.S + a.n_hi;
    const size_t lds = (size_t)NW * MTW * NTW * 16 * 64 * sizeof(float);
    if (NTW > 1 && (a.NT % NTW != 0 || a.S != 1 || a.n_hi != 0)) { set_error("k_gemm: %d column tiles per workgroup need S == 1 and NT %% %d == 0", NTW, NTW); return WMAR_EINVAL; }
    if (lds > 64 * 1024) {      // more than the default dynamic LDS limit: opt in once per instantiation
        static bool done = false;
        if (!done) { (void)hipFuncSetAttribute((const void*)k_gemm<MTW, NW, EPI, LN, ABL, U, ROT, NTW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); done = true; }
    }
    hipLaunchKernelGGL((k_gemm<MTW, NW, EPI, LN, ABL, U, ROT, NTW>), dim3((unsigned)grid), dim3(NW * 64), lds, st, a);
    return launch_status("k_gemm");
}

// Split-K factor for a GEMM whose partial slabs are folded by a later kernel: pick the S that
// fills the 256 CUs most evenly (whole "rounds" of workgroups), keeping >= 8 k-blocks per wave.
inline int pick_split(int tiles, int KB, int NW) {
    int best = 1;
    double best_eff = 0.0;
    for (int S = 1; S <= MAX_SLABS; ++S) {
        if (KB / (S * NW) < 8 && S > 1) break;
        const int wgs = tiles * S;
        const int rounds = (wgs + 255) / 256;
        const double eff = (double)wgs / (rounds * 256.0);
        if (eff > best_eff + 0.02) { best_eff = eff; best = S; }
    }
    return best;
}

// Row tiles per workgroup: two 32-row tiles share every weight fragment (half the operand
// traffic per MFMA); a single tile when the batch has only one.
// four row tiles per workgroup once two would need more than one workgroup per CU: a second
// workgroup on a CU shares its MFMA pipes, so the launch takes as long as the busiest CU
inline int gemm_row_tiles(int MT, int NT) { return (MT % 4 == 0 && NT * (MT / 2) > 256) ? 4 : (MT % 2 == 0 ? 2 : 1); }

template <int EPI, bool LN>
int gemm_dispatch(GemmArgs a, bool allow_split, hipStream_t st) {
    constexpr int NW = 4;
    if (gemm_row_tiles(a.MT, a.NT) == 4) {
        a.S = allow_split ? pick_split(a.NT * (a.MT / 4), a.KB, NW) : 1;
        return launch_gemm<4, NW, EPI, LN, 0, 2>(a, st);
    }
    if (a.MT % 2 == 0) {
        a.S = allow_split ? pick_split(a.NT * (a.MT / 2), a.KB, NW) : 1;
        return launch_gemm<2, NW, EPI, LN>(a, st);
    }
    a.S = allow_split ? pick_split(a.NT * a.MT, a.KB, NW) : 1;
    return launch_gemm<1, NW, EPI, LN>(a, st);
}

// row tiles per workgroup of gemm_split's k_gemm
inline int gemm_split_row_tiles(int MT) { return MT % 2 == 0 ? 2 : 1; }

// split-K GEMM writing partial slabs; reports the S it used
inline int gemm_split(GemmArgs a, int* S_out, hipStream_t st, int force_S = 0) {
    constexpr int NW = 4;
    if (gemm_split_row_tiles(a.MT) == 2) {
        a.S = force_S > 0 ? force_S : pick_split(a.NT * (a.MT / 2), a.KB, NW);
        *S_out = a.S;
        return launch_gemm<2, NW, EPI_PACKED, false>(a, st);
    }
    a.S = force_S > 0 ? force_S : pick_split(a.NT * a.MT, a.KB, NW);
    *S_out = a.S;
    return launch_gemm<1, NW, EPI_PACKED, false>(a, st);
}

// chunks of <= STAT_CHUNK k-blocks: one k_resid_stats workgroup (4 waves x up to 4 blocks) per chunk and row tile
constexpr int STAT_CHUNK = 16;
inline int stat_chunks(int KB) { const int n = (KB + STAT_CHUNK - 1) / STAT_CHUNK; return n <= STAT_CHUNKS_MAX ? n : (KB + 15) / 16; }


// Captured graphs of one engine: N graph / exec slots on one capture stream, and the rule for their lifetime -- an exec that may
// still be replaying (`pending`, until the `done` event recorded behind the last replays has passed) is waited for before it is
// destroyed, and a capture that fails leaves no graph behind.  Which slot is captured when, and when graphs are reused, is the
// policy of gen_loop.h.  Declared BEHIND the engine's DeviceArena, so that the graphs are dropped before the memory they use is freed.
template <int N>
struct GraphSlots {
    static constexpr int n_slots = N;
    hipStream_t cap = nullptr;
    hipEvent_t done = nullptr;
    hipGraph_t graph[N] = {};
    hipGraphExec_t exec[N] = {};
    bool pending = false;
    int64_t captures = 0;        // successful capture() calls since creation: tells a reuse from a recapture (wmar_*_graph_counts)
    bool has(int slot) const { return exec[slot] != nullptr; }
    int init() {
        WMAR_HIP_CHECK(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
        WMAR_HIP_CHECK(hipEventCreate(&done));
        return WMAR_OK;
    }
    void drop() {
        if (pending && done) (void)hipEventSynchronize(done);
        pending = false;
        for (int i = 0; i < N; ++i) {
            if (exec[i]) (void)hipGraphExecDestroy(exec[i]);
            if (graph[i]) (void)hipGraphDestroy(graph[i]);
            exec[i] = nullptr; graph[i] = nullptr;
        }
    }
    // slot <- the launches `enqueue(cap)` puts on the capture stream, instantiated.  On any failure every slot is dropped.
    template <typename F>
    int capture(int slot, F&& enqueue) {
        int rc = WMAR_OK;
        hipError_t e = hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) { set_error("hipStreamBeginCapture: %s", hipGetErrorString(e)); rc = WMAR_EHIP; }
        else {
            rc = enqueue(cap);
            e = hipStreamEndCapture(cap, &graph[slot]);      // ends the capture whatever `enqueue` returned
            if (rc == WMAR_OK && e != hipSuccess) { set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); rc = WMAR_EHIP; }
        }
        if (rc == WMAR_OK && (e = hipGraphInstantiate(&exec[slot], graph[slot], nullptr, nullptr, 0)) != hipSuccess) {
            set_error("hipGraphInstantiate: %s", hipGetErrorString(e)); rc = WMAR_EHIP;
        }
        if (rc != WMAR_OK) drop();
        else captures += 1;
        return rc;
    }
    int replay(int slot, hipStream_t st) {
        const hipError_t e = hipGraphLaunch(exec[slot], st);
        if (e != hipSuccess) { set_error("graph replay failed: %s", hipGetErrorString(e)); return WMAR_EHIP; }
        return WMAR_OK;
    }
    // behind the last replay of a call: from here on drop() waits for them
    int replayed(hipStream_t st) {
        const hipError_t e = hipEventRecord(done, st);
        if (e != hipSuccess) { set_error("graph replay failed: %s", hipGetErrorString(e)); return WMAR_EHIP; }
        pending = true;
        return WMAR_OK;
    }
    GraphSlots() = default;
    GraphSlots(const GraphSlots&) = delete;
    GraphSlots& operator=(const GraphSlots&) = delete;
    ~GraphSlots() {
        drop();
        if (cap) (void)hipStreamDestroy(cap);
        if (done) (void)hipEventDestroy(done);
    }
};

// Can every workgroup of a `blocks`-wide grid be resident at once?  (What the device holds: workgroups per compute unit x the
// compute units the runtime exposes -- a CU mask or a partition mode shrinks it.)  Kernels whose workgroups wait for each other
// inside one launch need it; a query that fails counts as "no".
inline bool grid_resident(int blocks_per_cu, long long blocks) {
    int dev = 0, cus = 0;
    return hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
           (long long)blocks_per_cu * cus >= blocks;
}
template <typename Kernel>
bool grid_resident(Kernel kernel, int threads, long long blocks) {
    int nb = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, 0) == hipSuccess && grid_resident(nb, blocks);
}

// Do the blocks of a `blocks`-wide grid with equal blockIdx % 8 share an XCD, the eight groups on eight different ones?  Three
// launches of k_xcc_probe: the id a group gets rotates with the launches before it, the grouping must not.
inline bool xcd_grouping_ok(int blocks, int threads, hipStream_t st) {
    unsigned* tmp = nullptr;
    std::vector<unsigned> h((size_t)blocks);
    bool ok = hipMalloc(&tmp, (size_t)blocks * 4) == hipSuccess;
    for (int rep = 0; rep < 3 && ok; ++rep) {
        hipLaunchKernelGGL(k_xcc_probe, dim3((unsigned)blocks), dim3((unsigned)threads), 0, st, tmp);
        ok = hipMemcpyAsync(h.data(), tmp, (size_t)blocks * 4, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        unsigned seen = 0;
        for (int b = 0; b < blocks && ok; ++b) ok = h[b] == h[b & 7] && h[b] < 16;
        for (int x = 0; x < 8 && ok; ++x) { ok = !(seen & (1u << h[x])); seen |= 1u << h[x]; }
    }
    if (tmp) (void)hipFree(tmp);
    return ok;
}

// Work that may run a launch with an in-launch barrier: `run()` enqueues it, `failed()` then reads the barrier's flag (the engine's
// *_sync_failed: 1 = the flag was up and the engine has switched to its fallback path, < 0 = error).  A failed run is repeated
// once -- on the fallback path, where the flag cannot come up; `still_up` is the error text if it does.
template <typename Run, typename Failed>
int run_with_fallback(const char* still_up, Run&& run, Failed&& failed) {
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (int rc = run()) return rc;
        const int f = failed();
        if (f <= 0) return f;
    }
    set_error("%s", still_up);
    return WMAR_EHIP;
}

// the tail of a generation step: the sampler, then pos, step and len (ctr[0..3)) move on by one
inline int advance3(int* ctr, hipStream_t st) {
    hipLaunchKernelGGL(k_advance3, dim3(1), dim3(1), 0, st, ctr);
    return launch_status("k_advance3");
}
inline int sample_then_advance(const SampArgs& a, int* ctr, hipStream_t st) {
    if (int rc = launch_sample_fused(a, st)) return rc;
    return advance3(ctr, st);
}

}  // namespace wmar
