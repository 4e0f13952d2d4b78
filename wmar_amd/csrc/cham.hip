// Chameleon / Anole decode engine for gfx950 (bf16 weights and activations, fp32 accumulation)
// -- SURVEY.md section 8a row C1.
//
// Reference: deps/chameleon/inference/transformer.py:288-353 (Transformer.forward_with_attn_bias),
// :37-160 (Attention), :163-217 (FeedForward), :220-285 (TransformerBlock, swin_norm = False);
// model_adapter.py:72-119 (ragged prefill, then one token per sequence per step);
// chameleon.py:299-389 (ImageDecoder: three guidance streams, 1024 image tokens);
// logits_processor.py:312-336 (InBatchInstructCFG), :135-156 (AllowOnlyTokens);
// token_selector.py:26-47 (multinomial on the first stream, replicated).
//
// One step = every row (sequence) consumes one token at its own position: the prompt is fed
// token by token through the same captured step (prompts are a few dozen tokens against 1024
// generated ones), rows of shorter prompts idle until their turn (AlignPromptRight).
#include <cmath>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "cham_kernels.h"
#include "probe_host.h"
#include "sampler.h"

namespace wmar {

struct ChamLayer {
    uint4 *wqkv, *wo, *w13, *w2;
    float *qnw, *qnb, *knw, *knb;
};

}  // namespace wmar

using namespace wmar;

struct wmar_cham {
    wmar_cham_config cfg{};
    DeviceArena mem;
    int D = 0, H = 0, Hkv = 0, hd = 0, V = 0, L = 0, F = 0, T = 0, Mmax = 0, MT = 0, Dkv = 0;
    std::vector<ChamLayer> layers;
    uint16_t* emb = nullptr;
    uint4* whead = nullptr;
    // workspaces
    uint4 *x = nullptr, *y = nullptr, *hbuf = nullptr;
    float *slabs = nullptr, *big_slabs = nullptr, *logits = nullptr, *scratch = nullptr;   // pieces of D-wide / of QKV and w13 outputs
    double* ssq = nullptr;
    uint16_t *kcache = nullptr, *vcache = nullptr;
    long long *tok = nullptr, *ids = nullptr;
    float2* rope = nullptr;
    int *pos = nullptr, *ctr = nullptr;     // ctr: [unused, step, len]
    // wmar_cham_generate_image waits for its stream before it returns (it frees the prompt tables): no replay outlives the call.
    // The shared loops (gen_loop.h) mark the graphs as replaying all the same; the drop() that then waits finds the event passed.
    GraphSlots<1> gr;
    // hooked generation (wmar_cham_generate_image_hooked): graph A (token bookkeeping + model step + guidance mix) and graph B
    // (sampler + counters) in slots and under a key of their own: kept across calls, untouched by the fused calls
    GraphSlots<2> grh;
    GraphKey hook_key;
};

namespace {

// workgroups of the stream-K GEMM: one per CU (measured: 256 -> 5.3 ms/step, 512 -> 5.9, 1024 -> 6.5 on the 7B model; the kernel
// runs at one wave per SIMD, so more workgroups only add pieces and prologues).  Dev builds (-DWMAR_DEV_KNOBS): WMAR_CHAM_GRID overrides.
int cham_grid() {
#ifdef WMAR_DEV_KNOBS
    static int g = 0;
    if (!g) {
        const char* e = getenv("WMAR_CHAM_GRID");
        g = e ? atoi(e) : 256;
        if (g < 1) g = 256;
    }
    return g;
#else
    return 256;
#endif
}

SkInfo sk_for(int NT, int KB, bool whole_groups) {
    SkInfo k;
    const int groups = (NT + BG_TG - 1) / BG_TG;
    k.C = (KB + BG_KC - 1) / BG_KC;
    k.U = groups * k.C;
    const int target = cham_grid();
    if (whole_groups) {
        // every workgroup owns whole groups: the largest grid <= target that divides the group count
        int per = (groups + target - 1) / target;
        while (groups % per) ++per;
        k.G = groups / per;
    } else {
        // at most BG_MAXP pieces per group (the slab buffers are sized for that)
        auto max_pieces = [&](int G) {
            SkInfo t = k;
            t.G = G;
            int mx = 0;
            for (int g = 0; g < groups; ++g) mx = std::max(mx, sk_count(t, g));
            return mx;
        };
        k.G = std::min(target, k.U);
        while (k.G > 1 && max_pieces(k.G) > BG_MAXP) k.G -= (k.G > 64 ? 16 : 1);
    }
    return k;
}

template <int EPI>
int launch_bgemm(const BGemmArgs& a, int MT, hipStream_t st) {
    const dim3 grid((unsigned)a.sk.G);
    switch (MT) {
        case 1: hipLaunchKernelGGL((k_bgemm<1, EPI>), grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL((k_bgemm<2, EPI>), grid, dim3(256), 0, st, a); break;
        case 3: hipLaunchKernelGGL((k_bgemm<3, EPI>), grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((k_bgemm<4, EPI>), grid, dim3(256), 0, st, a); break;
    }
    return launch_status("k_bgemm");
}

struct ChamPlan {
    wmar_cham* g;
    int M;
    hipStream_t st;
    int MT, KBD, KBF, nch;
    long long act8;     // floats per fp32 piece of a D-wide output
    SkInfo sk_qkv, sk_o, sk_13, sk_2, sk_head;
    ChamPlan(wmar_cham* g_, int M_, hipStream_t st_) : g(g_), M(M_), st(st_) {
        MT = g->MT; KBD = g->D / 16; KBF = g->F / 16; nch = (KBD + CHAM_STAT_KB - 1) / CHAM_STAT_KB;      // (<= 128: checked at creation)
        act8 = (long long)g->D * MT * 32;
        sk_qkv = sk_for((g->D + 2 * g->Dkv) / 32, KBD, false);
        sk_o = sk_for(g->D / 32, KBD, false);
        sk_13 = sk_for(g->F / 16, KBD, false);
        sk_2 = sk_for(g->D / 32, KBF, false);
        sk_head = sk_for(g->V / 32, KBD, true);
    }
    BGemmArgs base() const {
        BGemmArgs a{};
        a.M = M; a.ssq = g->ssq; a.n_chunks = nch; a.K = g->D; a.eps = g->cfg.norm_eps;
        return a;
    }
    int embed() {
        ChamResidArgs r{};
        r.x = g->x; r.emb = g->emb; r.tok = g->tok; r.ssq = g->ssq; r.KB = KBD; r.MT = MT; r.M = M; r.K = g->D;
        hipLaunchKernelGGL((k_cham_resid<true>), dim3((unsigned)(nch * MT)), dim3(256), 0, st, r);
        return launch_status("k_cham_resid<embed>");
    }
    int resid(const SkInfo& sk) {
        ChamResidArgs r{};
        r.x = g->x; r.slabs = g->slabs; r.slab_stride = act8; r.sk = sk; r.ssq = g->ssq; r.KB = KBD; r.MT = MT; r.M = M; r.K = g->D;
        hipLaunchKernelGGL((k_cham_resid<false>), dim3((unsigned)(nch * MT)), dim3(256), 0, st, r);
        return launch_status("k_cham_resid");
    }
    // the launches of one block, one member per stage (wmar_cham_probe_run runs them one at a time; layer() is their sequence)
    long long qkv_stride() const { return (long long)(g->D + 2 * g->Dkv) * MT * 32; }
    long long w13_stride() const { return (long long)2 * g->F * MT * 32; }
    int qkv(int l) {
        const int Nqkv = g->D + 2 * g->Dkv;
        BGemmArgs q = base();
        q.Wp = g->layers[l].wqkv; q.Xp = g->x; q.KB = KBD; q.NT = Nqkv / 32; q.sk = sk_qkv; q.slabs = g->big_slabs;
        q.slab_stride = qkv_stride();
        return launch_bgemm<BEPI_SLAB>(q, MT, st);
    }
    static int att_nw() {
        static const int nw = getenv("WMAR_CHAM_NWA") ? atoi(getenv("WMAR_CHAM_NWA")) : 2;     // dev A/B: waves per (sequence, head)
        return nw;
    }
    int attn(int l) {
        const ChamLayer& w = g->layers[l];
        ChamAttnArgs t{};
        const long long lstride = (long long)g->Mmax * g->Hkv * g->T * g->hd;
        t.qkv_slabs = g->big_slabs; t.slab_stride = qkv_stride(); t.sk = sk_qkv; t.ssq = g->ssq; t.n_chunks = nch; t.K = g->D;
        t.eps = g->cfg.norm_eps; t.qn_w = w.qnw; t.qn_b = w.qnb; t.kn_w = w.knw; t.kn_b = w.knb;
        t.kcache = g->kcache + l * lstride; t.vcache = g->vcache + l * lstride; t.y = g->y; t.pos = g->pos;
        t.D = g->D; t.H = g->H; t.Hkv = g->Hkv; t.Tmax = g->T; t.MT = MT; t.scale = 1.0f / sqrtf((float)g->hd);
        t.rope = g->rope;
        const dim3 grid((unsigned)(M * g->H));
        if (g->hd == 128 && att_nw() == 1) hipLaunchKernelGGL((k_cham_attn<128, 1>), grid, dim3(64), 0, st, t);
        else if (g->hd == 128 && att_nw() == 4) hipLaunchKernelGGL((k_cham_attn<128, 4>), grid, dim3(256), 0, st, t);
        else if (g->hd == 128) hipLaunchKernelGGL((k_cham_attn<128, 2>), grid, dim3(128), 0, st, t);
        else hipLaunchKernelGGL((k_cham_attn<64, 2>), grid, dim3(128), 0, st, t);
        return launch_status("k_cham_attn");
    }
    int wo(int l) {
        BGemmArgs o = base();
        o.Wp = g->layers[l].wo; o.Xp = g->y; o.KB = KBD; o.NT = g->D / 32; o.sk = sk_o; o.slabs = g->slabs; o.slab_stride = act8;
        return launch_bgemm<BEPI_SLAB>(o, MT, st);
    }
    int w13(int l) {
        BGemmArgs f = base();
        f.Wp = g->layers[l].w13; f.Xp = g->x; f.KB = KBD; f.NT = g->F / 16; f.sk = sk_13; f.slabs = g->big_slabs;
        f.slab_stride = w13_stride();
        return launch_bgemm<BEPI_SLAB>(f, MT, st);
    }
    int swiglu() {
        SwigluArgs sw{};
        sw.slabs = g->big_slabs; sw.slab_stride = w13_stride(); sw.sk = sk_13; sw.out = g->hbuf; sw.ssq = g->ssq; sw.n_chunks = nch;
        sw.K = g->D; sw.eps = g->cfg.norm_eps; sw.NT = g->F / 16; sw.MT = MT;
        hipLaunchKernelGGL(k_cham_swiglu, dim3((unsigned)((sw.NT + 3) / 4), (unsigned)MT), dim3(256), 0, st, sw);
        return launch_status("k_cham_swiglu");
    }
    int w2(int l) {
        BGemmArgs d = base();
        d.Wp = g->layers[l].w2; d.Xp = g->hbuf; d.KB = KBF; d.NT = g->D / 32; d.sk = sk_2; d.slabs = g->slabs; d.slab_stride = act8;
        return launch_bgemm<BEPI_SLAB>(d, MT, st);
    }
    int layer(int l) {
        int rc;
        if ((rc = qkv(l))) return rc;
        if ((rc = attn(l))) return rc;
        if ((rc = wo(l))) return rc;
        if ((rc = resid(sk_o))) return rc;
        if ((rc = w13(l))) return rc;
        if ((rc = swiglu())) return rc;
        if ((rc = w2(l))) return rc;
        return resid(sk_2);
    }
    int head(float* logits_out) {
        BGemmArgs a = base();
        a.Wp = g->whead; a.Xp = g->x; a.KB = KBD; a.NT = g->V / 32; a.sk = sk_head; a.logits = logits_out; a.V = g->V;
        return launch_bgemm<BEPI_LOGITS>(a, MT, st);
    }
    int step(bool with_head, float* logits_out) {
        int rc;
        if ((rc = embed())) return rc;
        for (int l = 0; l < g->L; ++l)
            if ((rc = layer(l))) return rc;
        return with_head ? head(logits_out) : WMAR_OK;
    }
};

int bpack(const void* src, const void* gamma, uint4* dst, int N, int K, int mode, int Hd, int src_bf16, hipStream_t st) {
    BPackArgs a{};
    a.src = src; a.gamma = gamma; a.dst = dst; a.N = N; a.K = K; a.mode = mode; a.Hd = Hd; a.src_bf16 = src_bf16;
    const int NT = mode == 0 ? (N + 31) / 32 : Hd / 16;
    hipLaunchKernelGGL(k_bpack, dim3((unsigned)((long long)NT * (K / 16))), dim3(64), 0, st, a);
    return launch_status("k_bpack");
}

}  // namespace

extern "C" {

int wmar_cham_create(const wmar_cham_config* cfg, const char* const* names, const void* const* tensors_dev,
                     int32_t n_tensors, void* stream, wmar_cham** out) {
    WMAR_REQUIRE(cfg && names && tensors_dev && out, "cham_create: null argument");
    const int D = cfg->dim, H = cfg->n_heads, Hkv = cfg->n_kv_heads, L = cfg->n_layers, F = cfg->ffn_hidden, V = cfg->vocab_size;
    WMAR_REQUIRE(H > 0 && Hkv > 0 && D % H == 0 && H % Hkv == 0, "cham_create: bad head counts");
    const int hd = D / H;
    WMAR_REQUIRE(hd == 64 || hd == 128, "cham_create: head_dim %d unsupported (64, 128)", hd);
    WMAR_REQUIRE(D % 32 == 0 && F % 16 == 0 && V % 32 == 0 && (Hkv * hd) % 16 == 0, "cham_create: dim / ffn / vocab alignment");
    WMAR_REQUIRE(!cfg->swin_norm, "cham_create: swin_norm (Chameleon-30B block order) is not supported");
    WMAR_REQUIRE(cfg->max_rows >= 1 && cfg->max_rows <= 128, "cham_create: max_rows must be in 1..128");
    WMAR_REQUIRE(cfg->max_seq_len >= 2, "cham_create: max_seq_len too small");
    WMAR_REQUIRE((D / 16 + CHAM_STAT_KB - 1) / CHAM_STAT_KB <= 128, "cham_create: dim %d gives more than 128 statistics chunks (k_cham_attn reads two per lane)", D);
    TensorMap tm(names, tensors_dev, n_tensors);
    hipStream_t st = (hipStream_t)stream;
    auto* g = new wmar_cham();
    g->cfg = *cfg; g->D = D; g->H = H; g->Hkv = Hkv; g->hd = hd; g->V = V; g->L = L; g->F = F; g->Dkv = Hkv * hd;
    g->T = cfg->max_seq_len; g->Mmax = cfg->max_rows; g->MT = (cfg->max_rows + 31) / 32;
    const int bf = cfg->tensors_bf16;
    int& rc = tm.rc;
    auto vec_f32 = [&](float** dst, const void* src, size_t n) -> int {
        if (int r = g->mem.alloc(dst, n)) return r;
        hipLaunchKernelGGL(k_to_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, *dst, (long long)n, bf);
        return launch_status("k_to_f32");
    };
    const void *e = tm.need("tok_embeddings.weight"), *nw = tm.need("norm.weight"), *ow = tm.need("output.weight");
    if (rc == WMAR_OK) {
        WMAR_TRY(g->mem.alloc(&g->emb, (size_t)V * D));
        if (rc == WMAR_OK) {
            const long long n = (long long)V * D;
            hipLaunchKernelGGL(k_to_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, e, g->emb, n, bf);
            rc = launch_status("k_to_bf16");
        }
        WMAR_TRY(g->mem.alloc(&g->whead, (size_t)V * D / 8));
        WMAR_TRY(bpack(ow, nw, g->whead, V, D, 0, 0, bf, st));
    }
    g->layers.resize(L);
    const int Nqkv = D + 2 * g->Dkv;
    for (int l = 0; l < L && rc == WMAR_OK; ++l) {
        const std::string p = "layers." + std::to_string(l) + ".";
        ChamLayer& w = g->layers[l];
        const void *qkv = tm.need(p + "attention.wqkv.weight"), *wo = tm.need(p + "attention.wo.weight"),
                   *w13 = tm.need(p + "feed_forward.w13.weight"), *w2 = tm.need(p + "feed_forward.w2.weight"),
                   *an = tm.need(p + "attention_norm.weight"), *fn = tm.need(p + "ffn_norm.weight");
        const void *qw = nullptr, *qb = nullptr, *kw = nullptr, *kb = nullptr;
        if (cfg->qk_normalization) {
            qw = tm.need(p + "attention.q_normalization.weight"); qb = tm.need(p + "attention.q_normalization.bias");
            kw = tm.need(p + "attention.k_normalization.weight"); kb = tm.need(p + "attention.k_normalization.bias");
        }
        if (rc != WMAR_OK) break;
        WMAR_TRY(g->mem.alloc(&w.wqkv, (size_t)Nqkv * D / 8)); WMAR_TRY(bpack(qkv, an, w.wqkv, Nqkv, D, 0, 0, bf, st));
        WMAR_TRY(g->mem.alloc(&w.wo, (size_t)D * D / 8)); WMAR_TRY(bpack(wo, nullptr, w.wo, D, D, 0, 0, bf, st));
        WMAR_TRY(g->mem.alloc(&w.w13, (size_t)2 * F * D / 8)); WMAR_TRY(bpack(w13, fn, w.w13, 2 * F, D, 1, F, bf, st));
        WMAR_TRY(g->mem.alloc(&w.w2, (size_t)D * F / 8)); WMAR_TRY(bpack(w2, nullptr, w.w2, D, F, 0, 0, bf, st));
        w.qnw = w.qnb = w.knw = w.knb = nullptr;
        if (cfg->qk_normalization) {
            WMAR_TRY(vec_f32(&w.qnw, qw, (size_t)hd)); WMAR_TRY(vec_f32(&w.qnb, qb, (size_t)hd));
            WMAR_TRY(vec_f32(&w.knw, kw, (size_t)hd)); WMAR_TRY(vec_f32(&w.knb, kb, (size_t)hd));
        }
    }
    const size_t Mpad = (size_t)g->MT * 32;
    WMAR_TRY(g->mem.alloc_zero(&g->x, Mpad * D / 8, st));
    WMAR_TRY(g->mem.alloc_zero(&g->y, Mpad * D / 8, st));
    WMAR_TRY(g->mem.alloc_zero(&g->hbuf, Mpad * F / 8, st));
    WMAR_TRY(g->mem.alloc_zero(&g->slabs, (size_t)BG_MAXP * Mpad * D, st));                       // padding rows are never written
    WMAR_TRY(g->mem.alloc_zero(&g->big_slabs, (size_t)BG_MAXP * Mpad * (size_t)std::max(Nqkv, 2 * F), st));
    WMAR_TRY(g->mem.alloc(&g->ssq, (size_t)((D / 16 + CHAM_STAT_KB - 1) / CHAM_STAT_KB) * Mpad));
    const size_t kv = (size_t)L * g->Mmax * Hkv * g->T * hd;
    WMAR_TRY(g->mem.alloc_zero(&g->kcache, kv, st));
    WMAR_TRY(g->mem.alloc_zero(&g->vcache, kv, st));
    WMAR_TRY(g->mem.alloc(&g->logits, (size_t)g->Mmax * V));
    WMAR_TRY(g->mem.alloc(&g->scratch, (size_t)g->Mmax * V));
    WMAR_TRY(g->mem.alloc_zero(&g->tok, Mpad, st));
    WMAR_TRY(g->mem.alloc_zero(&g->pos, Mpad, st));
    WMAR_TRY(g->mem.alloc(&g->ids, (size_t)g->Mmax * (size_t)(g->T + 4)));
    WMAR_TRY(g->mem.alloc_zero(&g->ctr, 4, st));
    WMAR_TRY(g->mem.alloc(&g->rope, (size_t)g->T * (hd / 2)));
    if (rc == WMAR_OK) {
        const long long n = (long long)g->T * (hd / 2);
        hipLaunchKernelGGL(k_rope_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g->rope, g->T, hd / 2, cfg->rope_theta);
        rc = launch_status("k_rope_table");
    }
    WMAR_TRY(g->gr.init());
    WMAR_TRY(g->grh.init());
    if (rc == WMAR_OK) {
        const hipError_t er = hipStreamSynchronize(st);
        if (er != hipSuccess) { set_error("cham_create: %s", hipGetErrorString(er)); rc = WMAR_EHIP; }
    }
    if (rc != WMAR_OK) { delete g; return rc; }
    *out = g;
    return WMAR_OK;
}

void wmar_cham_destroy(wmar_cham* g) { delete g; }
int64_t wmar_cham_device_bytes(const wmar_cham* g) { return g ? g->mem.bytes : 0; }
int wmar_cham_graph_counts(const wmar_cham* g, int64_t* fused, int64_t* hooked) {
    WMAR_REQUIRE(g, "cham_graph_counts: null argument");
    if (fused) *fused = g->gr.captures;
    if (hooked) *hooked = g->grh.captures;
    return WMAR_OK;
}

int wmar_cham_forward_tokens(wmar_cham* g, const int64_t* tok_dev, const int32_t* pos_dev, int64_t M, float* logits_dev,
                             void* stream) {
    WMAR_REQUIRE(g && tok_dev && pos_dev, "cham_forward_tokens: null argument");
    WMAR_REQUIRE(M >= 1 && M <= g->Mmax, "cham_forward_tokens: rows %lld outside 1..%d", (long long)M, g->Mmax);
    hipStream_t st = (hipStream_t)stream;
    WMAR_HIP_CHECK(hipMemcpyAsync(g->tok, tok_dev, (size_t)M * 8, hipMemcpyDeviceToDevice, st));
    WMAR_HIP_CHECK(hipMemcpyAsync(g->pos, pos_dev, (size_t)M * 4, hipMemcpyDeviceToDevice, st));
    ChamPlan p(g, (int)M, st);
    return p.step(logits_dev != nullptr, logits_dev);
}

// ---------------------------------------------------------------------------------------------- test-only stage access
int wmar_cham_probe_run(wmar_cham* g, const int64_t* tok_dev, const int32_t* pos_dev, int64_t M, int32_t layer, int32_t first_stage,
                        int32_t last_stage, float* logits_dev, void* stream) {
    WMAR_REQUIRE(g, "cham_probe_run: null engine");
    WMAR_REQUIRE(M >= 1 && M <= g->Mmax, "cham_probe_run: rows %lld outside 1..%d", (long long)M, g->Mmax);
    WMAR_REQUIRE(layer >= 0 && layer < g->L, "cham_probe_run: layer %d outside 0..%d", layer, g->L - 1);
    if (int rc = probe_stage_range("cham_probe_run", first_stage, last_stage, WMAR_CHAM_STAGE_HEAD, logits_dev)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (first_stage == WMAR_CHAM_STAGE_EMBED) {
        WMAR_REQUIRE(tok_dev && pos_dev, "cham_probe_run: the EMBED stage needs tok_dev and pos_dev");
        WMAR_HIP_CHECK(hipMemcpyAsync(g->tok, tok_dev, (size_t)M * 8, hipMemcpyDeviceToDevice, st));
        WMAR_HIP_CHECK(hipMemcpyAsync(g->pos, pos_dev, (size_t)M * 4, hipMemcpyDeviceToDevice, st));
    }
    ChamPlan p(g, (int)M, st);
    int rc = WMAR_OK;
    for (int s = first_stage; s <= last_stage && rc == WMAR_OK; ++s) {
        switch (s) {
            case WMAR_CHAM_STAGE_EMBED: rc = p.embed(); break;
            case WMAR_CHAM_STAGE_QKV: rc = p.qkv(layer); break;
            case WMAR_CHAM_STAGE_ATTN: rc = p.attn(layer); break;
            case WMAR_CHAM_STAGE_WO: rc = p.wo(layer); break;
            case WMAR_CHAM_STAGE_RESID_ATTN: rc = p.resid(p.sk_o); break;
            case WMAR_CHAM_STAGE_W13: rc = p.w13(layer); break;
            case WMAR_CHAM_STAGE_SWIGLU: rc = p.swiglu(); break;
            case WMAR_CHAM_STAGE_W2: rc = p.w2(layer); break;
            case WMAR_CHAM_STAGE_RESID_FFN: rc = p.resid(p.sk_2); break;
            default: rc = p.head(logits_dev); break;
        }
    }
    return probe_wait("cham_probe_run", rc, st);
}

int64_t wmar_cham_probe_copy(wmar_cham* g, const char* name, int32_t layer, void* ptr_dev, int64_t bytes, int32_t to_engine,
                             void* stream) {
    if (!g || !name) { set_error("cham_probe_copy: null argument"); return WMAR_EINVAL; }
    if (layer < 0 || layer >= g->L) { set_error("cham_probe_copy: layer %d outside 0..%d", layer, g->L - 1); return WMAR_EINVAL; }
    const size_t Mpad = (size_t)g->MT * 32, D = g->D, F = g->F, Nqkv = (size_t)g->D + 2 * g->Dkv;
    const size_t lkv = (size_t)g->Mmax * g->Hkv * g->T * g->hd;
    const ChamLayer& w = g->layers[layer];
    const ProbeBuf bufs[] = {
        {"x", g->x, Mpad * D * 2},
        {"y", g->y, Mpad * D * 2},
        {"hbuf", g->hbuf, Mpad * F * 2},
        {"slabs", g->slabs, (size_t)BG_MAXP * Mpad * D * 4},
        {"big_slabs", g->big_slabs, (size_t)BG_MAXP * Mpad * std::max(Nqkv, 2 * F) * 4},
        {"ssq", g->ssq, (size_t)((D / 16 + CHAM_STAT_KB - 1) / CHAM_STAT_KB) * Mpad * 8},
        {"kcache", g->kcache + (size_t)layer * lkv, lkv * 2},
        {"vcache", g->vcache + (size_t)layer * lkv, lkv * 2},
        {"rope", g->rope, (size_t)g->T * (g->hd / 2) * 8},
        {"wqkv", w.wqkv, Nqkv * D * 2},
        {"wo", w.wo, D * D * 2},
        {"w13", w.w13, 2 * F * D * 2},
        {"w2", w.w2, D * F * 2},
        {"whead", g->whead, (size_t)g->V * D * 2},
    };
    return probe_copy("cham_probe_copy", bufs, sizeof bufs / sizeof *bufs, name, ptr_dev, bytes, to_engine, (hipStream_t)stream);
}

int wmar_cham_probe_plan(wmar_cham* g, int64_t M, char* buf, int64_t buf_len) {
    WMAR_REQUIRE(g && buf && buf_len > 0, "cham_probe_plan: null argument");
    WMAR_REQUIRE(M >= 1 && M <= g->Mmax, "cham_probe_plan: rows %lld outside 1..%d", (long long)M, g->Mmax);
    ChamPlan p(g, (int)M, nullptr);
    const int nw = g->hd == 128 && (ChamPlan::att_nw() == 1 || ChamPlan::att_nw() == 4) ? ChamPlan::att_nw() : 2;
    auto sk = [](const SkInfo& k) { return std::to_string(k.C) + "," + std::to_string(k.U) + "," + std::to_string(k.G); };
    const std::string t = "MT=" + std::to_string(p.MT) + " sk_qkv=" + sk(p.sk_qkv) + " sk_o=" + sk(p.sk_o) + " sk_13=" + sk(p.sk_13) +
                          " sk_2=" + sk(p.sk_2) + " sk_head=" + sk(p.sk_head) + " kernels=k_bgemm<" + std::to_string(p.MT) + ",SLAB>;k_bgemm<" +
                          std::to_string(p.MT) + ",LOGITS>;k_cham_attn<" + std::to_string(g->hd) + "," + std::to_string(nw) + ">";
    snprintf(buf, (size_t)buf_len, "%s", t.c_str());
    return WMAR_OK;
}

static int cham_generate_image(wmar_cham* g, const wmar_wm_ctx* wm, const int64_t* prompt_tokens_host,
                               const int32_t* prompt_lens_host, int64_t B, const wmar_cham_sample_params* sp,
                               const uint32_t* allow_dev, const int32_t* allow_ids_dev, int32_t n_allow, const float* q_dev,
                               int32_t n_tokens, int64_t* tokens_out_dev, void* stream, const HookIO* hk) {
    WMAR_REQUIRE(g && prompt_tokens_host && prompt_lens_host && sp && q_dev && tokens_out_dev, "cham_generate_image: null argument");
    WMAR_REQUIRE(B >= 1 && 3 * B <= g->Mmax, "cham_generate_image: batch %lld needs %lld rows, engine has %d", (long long)B,
                 (long long)(3 * B), g->Mmax);
    WMAR_REQUIRE(n_tokens >= 1, "cham_generate_image: n_tokens");
    WMAR_REQUIRE(!(sp->top_p >= 0) || sp->top_p <= 1.0, "`top_p` has to be a float > 0 and < 1, but is %f", sp->top_p);
    if (wm) WMAR_REQUIRE(wm->table_dev && wm->vocab_size == g->V, "cham_generate_image: watermark vocab mismatch");
    if (wm) WMAR_REQUIRE(wm->seed_strategy != WMAR_SEED_SPATIAL && wm->context_size <= 3,
                         "Chameleon supports fixed / linear seeding with context size <= 3 (generate.py of the reference: fixed / linear only)");
    hipStream_t st = (hipStream_t)stream;
    const int M = 3 * (int)B, V = g->V;
    int maxlen = 0;
    for (int m = 0; m < M; ++m) {
        WMAR_REQUIRE(prompt_lens_host[m] >= 1, "cham_generate_image: empty prompt in row %d", m);
        maxlen = std::max(maxlen, (int)prompt_lens_host[m]);
    }
    WMAR_REQUIRE(maxlen + n_tokens <= g->T, "cham_generate_image: %d prompt + %d image tokens exceed max_seq_len %d", maxlen,
                 n_tokens, g->T);
    if (hk) {
        WMAR_REQUIRE(hk->logits && hk->past && hk->hook && !wm, "cham_generate_image_hooked: null argument");
        WMAR_REQUIRE(hk->past_stride >= (long long)maxlen + n_tokens, "cham_generate_image_hooked: past_stride %lld below prompt %d + image tokens %d",
                     hk->past_stride, maxlen, n_tokens);
    } else {
        g->gr.drop();
    }
    // right-aligned prompt tables (alignment.py:27-52): row m idles (token 0 at position 0) until its prompt starts
    // the watermark sees the whole padded row: keep its last CTX entries (prompt tokens, pad_id where the row is still padding)
    // (hooked mode: the processor sees the whole padded row of the first stream, generation.py:86)
    const int CTX = hk ? maxlen : (maxlen < 3 ? maxlen : 3);
    const int CW = hk ? maxlen : 3;       // row width of first_ctx
    std::vector<long long> tt((size_t)maxlen * M), first_ctx((size_t)B * CW, 0);
    std::vector<int> tp((size_t)maxlen * M);
    size_t off = 0;
    for (int m = 0; m < M; ++m) {
        const int len = prompt_lens_host[m];
        for (int j = 0; j < maxlen; ++j) {
            const int i = j - (maxlen - len);
            const long long tk = i >= 0 ? prompt_tokens_host[off + i] : 0;
            WMAR_REQUIRE(tk >= 0 && tk < V, "cham_generate_image: prompt token %lld out of range", tk);
            tt[(size_t)j * M + m] = tk;
            tp[(size_t)j * M + m] = i >= 0 ? i : 0;
        }
        if (m < B)
            for (int c = 0; c < CTX; ++c) {
                const int i = len - CTX + c;
                first_ctx[(size_t)m * CW + c] = i >= 0 ? prompt_tokens_host[off + i] : (long long)sp->pad_id;
            }
        off += len;
    }
    long long* tab_tok = nullptr;
    int* tab_pos = nullptr;
    WMAR_HIP_CHECK(hipMalloc(&tab_tok, tt.size() * 8));
    if (hipMalloc(&tab_pos, tp.size() * 4) != hipSuccess) {
        (void)hipFree(tab_tok);
        set_error("cham_generate_image: out of device memory for the prompt tables");
        return WMAR_ENOMEM;
    }
    int rc = WMAR_OK;
    hipError_t e = hipMemcpyAsync(tab_tok, tt.data(), tt.size() * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(tab_pos, tp.data(), tp.size() * 4, hipMemcpyHostToDevice, st);
    // the watermark context is the whole input row: the tail of the padded prompt, then the generated tokens
    const long long ids_stride = hk ? hk->past_stride : g->T + 4;
    long long* ids = hk ? hk->past : g->ids;
    if (e == hipSuccess) e = hipMemcpy2DAsync(ids, ids_stride * 8, first_ctx.data(), (size_t)CW * 8, (size_t)CTX * 8, (size_t)B, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { set_error("cham_generate_image: %s", hipGetErrorString(e)); rc = WMAR_EHIP; }
    ChamPlan p(g, M, st);
    for (int j = 0; j < maxlen && rc == WMAR_OK; ++j) {
        hipLaunchKernelGGL(k_cham_step, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, st, g->tok, g->pos, tab_tok, tab_pos, j, M,
                           (const long long*)nullptr, 0ll, (const int*)nullptr, (int)B, 0);
        rc = p.step(j == maxlen - 1, g->logits);
    }
    hipLaunchKernelGGL(k_set3, dim3(1), dim3(1), 0, st, g->ctr, 0, 0, CTX);    // step = 0, len(ids row) = CTX
    if (rc == WMAR_OK) rc = launch_status("k_set3");

    SampArgs a = loop_samp_args(wm, hk ? hk->logits : g->logits, V, ids, ids_stride, g->ctr, sp->temperature, q_dev, B, g->scratch,
                                (long long*)tokens_out_dev, n_tokens);
    a.use_top_p = sp->top_p >= 0; a.top_p_thr = (float)(1.0 - sp->top_p);
    // hooked mode: the guidance mix has left the sampler (k_cfg_mix in front of the hook); allow-only and the row compaction stay
    // behind it (chameleon.py:313-327: CFG -> processors -> allow-only -> temperature -> top-p)
    if (!hk) { a.logits_img = g->logits + (long long)B * V; a.logits_uncond = g->logits + 2ll * B * V; }
    a.g_text = sp->guidance_scale_text; a.g_image = sp->guidance_scale_image; a.allow = allow_dev;
    if (allow_ids_dev && n_allow > 0) { a.gather = allow_ids_dev; a.Vsrc = V; a.V = n_allow; }

    auto sample = [&](hipStream_t s) { return sample_then_advance(a, g->ctr, s); };
    auto model_step = [&](hipStream_t s) -> int {    // consume the token sampled last -> logits of the next one
        hipLaunchKernelGGL(k_cham_step, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, s, g->tok, g->pos, (const long long*)nullptr,
                           (const int*)nullptr, 0, M, (const long long*)tokens_out_dev, (long long)n_tokens, (const int*)(g->ctr + 1),
                           (int)B, 1);
        ChamPlan q(g, M, s);
        return q.step(true, g->logits);
    };
    if (hk && rc == WMAR_OK) {
        CfgMixArgs mx{};
        mx.cond = g->logits; mx.img = g->logits + (long long)B * V; mx.uncond = g->logits + 2ll * B * V; mx.V = V; mx.B = B;
        mx.g_text = sp->guidance_scale_text; mx.g_image = sp->guidance_scale_image; mx.out = hk->logits;
        auto step_a = [&](hipStream_t s, int n) -> int {      // mixed logits of image token n: the first one from the prefill logits
            if (n > 0) { if (int r = model_step(s)) return r; }
            return launch_cfg_mix(mx, s);
        };
        GraphKey key;
        key.u64((uint64_t)B).u64((uint64_t)n_tokens).ptr(q_dev).ptr(tokens_out_dev).ptr(hk->logits).ptr(hk->past).u64((uint64_t)ids_stride);
        key.ptr(allow_dev).ptr(allow_ids_dev).i32(n_allow).f32(sp->temperature).f64(sp->top_p);
        key.f32(sp->guidance_scale_text).f32(sp->guidance_scale_image);
        rc = hooked_loop(g->grh, g->hook_key, key, sp->use_graph != 0, n_tokens, [](int n) { return n > 0 ? 0 : -1; }, step_a,
                         [&](int n) { return call_hook(*hk, n, (long long)maxlen + n); }, sample, st);
    } else if (rc == WMAR_OK) {
        // step 0 samples the first image token from the prefill logits, step n > 0 runs the model on the token sampled last.  Groups
        // of four steps per captured graph (the seam between two replays is ~10 us, gpt.hip); step 0 and the steps that do not fill
        // a group are enqueued directly in front of the replays.  Captured by every call.
        const int gs = 4, lead = 1 + (n_tokens - 1) % gs;
        rc = grouped_loop(g->gr, nullptr, GraphKey(), sp->use_graph != 0, n_tokens, lead, gs, [](int) { return 0; },
                          [&](hipStream_t s, int n) -> int {
                              if (n > 0) { if (int r = model_step(s)) return r; }
                              return sample(s);
                          }, st);
    }
    // the prompt tables are read by the prefill only; it has been enqueued on `st`, free after it ran
    hipError_t e2 = hipStreamSynchronize(st);
    (void)hipFree(tab_tok);
    (void)hipFree(tab_pos);
    if (rc == WMAR_OK && e2 != hipSuccess) { set_error("cham_generate_image: %s", hipGetErrorString(e2)); rc = WMAR_EHIP; }
    if (rc != WMAR_OK && !hk) g->gr.drop();
    if (rc != WMAR_OK && rc != WMAR_ECALLBACK && hk) g->grh.drop();
    return rc;
}

int wmar_cham_generate_image(wmar_cham* g, const wmar_wm_ctx* wm, const int64_t* prompt_tokens_host,
                             const int32_t* prompt_lens_host, int64_t B, const wmar_cham_sample_params* sp,
                             const uint32_t* allow_dev, const int32_t* allow_ids_dev, int32_t n_allow, const float* q_dev,
                             int32_t n_tokens, int64_t* tokens_out_dev, void* stream) {
    return cham_generate_image(g, wm, prompt_tokens_host, prompt_lens_host, B, sp, allow_dev, allow_ids_dev, n_allow, q_dev, n_tokens,
                               tokens_out_dev, stream, nullptr);
}

int wmar_cham_generate_image_hooked(wmar_cham* g, const int64_t* prompt_tokens_host, const int32_t* prompt_lens_host, int64_t B,
                                    const wmar_cham_sample_params* sp, const uint32_t* allow_dev, const int32_t* allow_ids_dev,
                                    int32_t n_allow, const float* q_dev, int32_t n_tokens, int64_t* tokens_out_dev,
                                    float* logits_io_dev, int64_t* past_io_dev, int64_t past_stride, wmar_logits_hook hook,
                                    void* user, void* stream) {
    // (this engine has no in-launch barrier: nothing to check behind the run, no re-run)
    const HookIO hk{logits_io_dev, (long long*)past_io_dev, (long long)past_stride, hook, user};
    return cham_generate_image(g, nullptr, prompt_tokens_host, prompt_lens_host, B, sp, allow_dev, allow_ids_dev, n_allow, q_dev,
                               n_tokens, tokens_out_dev, stream, &hk);
}

}  // extern "C"
