// Argument blocks shared by watermark.hip (kernels) and gpt.hip (generation graph).
#pragma once
#include "common.h"

namespace wmar {

struct WmDev {
    const uint32_t* table;
    long long n_rows;
    long long row_words;
    int seed_mode, h, S;
    float delta;
    int enabled;
};

inline WmDev make_wm(const wmar_wm_ctx* wm) {
    WmDev d{};
    if (wm) {
        d.table = wm->table_dev;
        d.n_rows = wm->n_rows;
        d.row_words = (wm->vocab_size + 31) / 32;
        d.seed_mode = wm->seed_strategy;
        d.h = wm->context_size;
        d.S = wm->spatial_dim;
        d.delta = wm->delta;
        d.enabled = 1;
    }
    return d;
}

struct SampArgs {
    WmDev wm;
    const float* logits;
    long long V;
    const long long* past;       // [B, past_stride]
    long long past_stride;
    long long t_host;            // used when t_dev == nullptr
    const int* t_dev;            // device-resident current length (generation graph)
    float temperature;
    int top_k;
    int use_top_p;
    float top_p_thr;             // (float)(1 - top_p)
    const float* q;              // [B, V]
    long long q_step_stride;     // elements between steps when q is indexed by *step_dev
    const int* step_dev;         // nullable
    float* scratch;              // [B, V]
    long long* tok_out;          // [B]
    long long tok_out_stride;    // tok_out[b*stride + step]
    long long* past_append;      // nullable: past[b*past_stride + t] = token
    float* trace;                // nullable: raw logits copy [steps][B][V]
    long long B;
    // classifier-free guidance (RAR.generate, rar.py:437-442): logits = uncond + (cond - uncond) * scale[step]
    const float* logits_uncond;  // nullable [B, V]
    const float* cfg_scale;      // device float [steps]
    // InBatchInstructCFG (deps/chameleon/inference/logits_processor.py:312-336): with logits_img set,
    // logits = uncond + g_image * (img - uncond) + g_text * (full - img); `logits` holds the fully conditioned rows
    const float* logits_img;     // nullable [B, V]
    float g_text, g_image;
    // AllowOnlyTokensLogitsProcessor (logits_processor.py:135-156): bit v clear -> logit v = -inf (after the watermark bias)
    const uint32_t* allow;       // nullable [V/32]
    // Row compaction: with `gather` (ascending source ids, int32 [V]) the row worked on is logits[gather[0..V)] -- exact
    // when every other entry would be -inf anyway (allow-only list); V is then the compact length, Vsrc the logits' width.
    // The token written is gather[argmax].
    const int* gather;           // nullable
    long long Vsrc;
};

int launch_sample_fused(const SampArgs& a, hipStream_t st);

// The sampler of a generation loop, as far as the engines agree: rows `logits` [B, V], the token row `past` the watermark reads and
// the sampler appends to, the counters ctr = [pos, step, len] on the device (noise and output column follow step, the append
// follows len), tok_out[b * tok_out_stride + step].  Guidance, top-k / top-p, trace, allow-only: the engine's own, set behind this.
inline SampArgs loop_samp_args(const wmar_wm_ctx* wm, const float* logits, long long V, long long* past, long long past_stride,
                               const int* ctr, float temperature, const float* q, long long B, float* scratch, long long* tok_out,
                               long long tok_out_stride) {
    SampArgs a{};
    a.wm = make_wm(wm);
    a.logits = logits; a.V = V; a.past = past; a.past_stride = past_stride; a.past_append = past;
    a.step_dev = ctr + 1; a.t_dev = ctr + 2;
    a.temperature = temperature; a.q = q; a.q_step_stride = B * V; a.B = B;
    a.scratch = V > 65536 ? scratch : nullptr;      // rows up to 65536 entries live in the sampler's registers
    a.tok_out = tok_out; a.tok_out_stride = tok_out_stride;
    return a;
}

// Guidance as a launch of its own (k_cfg_mix, watermark.hip): what k_sample_fused does to its rows in front of the watermark bias,
// written out as fp32 [B, V] -- the hooked generation mode hands that buffer to the host's logit processor.
struct CfgMixArgs {
    const float* cond;           // [B, V] conditional (RAR) / fully conditioned (Chameleon) rows
    const float* img;            // nullable [B, V]: image-conditioned rows -> the three-way form
    const float* uncond;         // [B, V]
    float* out;                  // [B, V]
    long long V, B;
    const float* scale;          // two-way: device float [steps], indexed by *step_dev (0 when step_dev is null)
    const int* step_dev;
    float g_text, g_image;       // three-way
};

int launch_cfg_mix(const CfgMixArgs& a, hipStream_t st);

// The host's side of a hooked generation (wmar_*_generate_hooked): its buffers and its callback.
struct HookIO {
    float* logits;               // [B, V]
    long long* past;             // [B, past_stride]
    long long past_stride;
    wmar_logits_hook hook;
    void* user;
};

// hook(user, step, t) between the two graphs of a step; non-zero -> WMAR_ECALLBACK
inline int call_hook(const HookIO& h, int step, long long t) {
    const int r = h.hook(h.user, (int32_t)step, (int64_t)t);
    if (r != 0) { set_error("the logits hook returned %d at step %d: generation stopped", r, step); return WMAR_ECALLBACK; }
    return WMAR_OK;
}

// Gumbel-key sampler (gumbel.hip): same step / append plumbing as SampArgs.
struct GumbelArgs {
    const float* logits;
    const float* logits_uncond;  // nullable (guidance, as above)
    const float* cfg_scale;
    const int* step_dev;         // nullable
    const int* t_dev;            // nullable: current length for past_append
    long long V, B;
    const float* log_rs;         // key rows: log_rs + b * key_row_stride
    long long key_row_stride;
    int use_sampling;
    float temp, top_p;
    int top_k;
    long long* tok_out;          // tok_out[b*tok_out_stride + step]
    long long tok_out_stride;
    long long* past_append;      // nullable: past_append[b*past_stride + t] = token
    long long past_stride;
};

int launch_gumbel_sample(const GumbelArgs& a, hipStream_t st);

// Key rows of one decode step of the context-keyed Gumbel watermark (gumbel.hip, k_gumbel_ctx_keys): row b of log_rs_out is
// log(rs) of the key hashed from the ngram ids in front of position *step_dev, or log(u[*step_dev, b]) while *step_dev < ngram.
struct GumbelCtxArgs {
    const long long* ids;        // [B, ids_stride] generated ids
    long long ids_stride;
    const int* step_dev;         // position being sampled
    unsigned long long h0;       // hash of the empty window
    int ngram;
    const float* u;              // [ngram, B, V] uniform noise of the unkeyed positions
    long long V, B;
    float* log_rs_out;           // [B, V]
};

int launch_gumbel_ctx_keys(const GumbelCtxArgs& a, hipStream_t st);

}  // namespace wmar
