/*
 * wmar_hip.h -- C ABI of libwmar_hip.so, the MI355X (gfx950) implementation of
 * wmar's watermarked autoregressive image generation + detection hot path.
 *
 * Conventions
 *   - plain C types only; every `*_dev` / "device" pointer is a HIP device pointer
 *     (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream).  Tensors stay owned by the caller.
 *   - every function returns 0 on success or a negative WMAR_E* code;
 *     wmar_last_error() returns a human-readable message for the calling thread.
 *   - engines allocate in *_create; afterwards only small per-call scratch is allocated (prompt tables of
 *     wmar_cham_generate_image, the one-off unconditional adaLN table of wmar_rar_generate, a status word of
 *     wmar_gumbel_score / wmar_gumbel_score_ctx); wmar_image_ingest keeps one scratch buffer per device between calls and
 *     grows it to the largest batch seen (coefficient tables + 8-bit intermediate: rows x target x 3 bytes per image).
 *   - an engine handle (wmar_gpt / wmar_rar / wmar_cham / wmar_vq / wmar_mvq) is NOT thread-safe: it owns
 *     its workspaces, KV cache and captured graphs; use it from one thread and one stream at a time
 *     (the reference is single-threaded per model too).
 *
 * Each entry point cites the reference interface (facebookresearch/wmar) it replaces.
 */
#ifndef WMAR_HIP_H
#define WMAR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WMAR_OK 0
#define WMAR_EINVAL (-1)   /* bad argument / unsupported shape            */
#define WMAR_EHIP (-2)     /* HIP runtime error                           */
#define WMAR_ESHORT (-3)   /* detect: len(codes) - context_size < 1       */
/* LINEAR / FIXED seeding take any context size up to this (gentime_watermark.py:236-241 has no limit; the key table has
 * context_size * (vocab - 1) + 1 rows of vocab / 8 bytes, so memory is the practical bound); SPATIAL: 1 or 3 as in the
 * reference (:243); the Chameleon generation loop keeps 3 prompt tokens in front of the image tokens: context_size <= 3 there. */
#define WMAR_MAX_CONTEXT 16
#define WMAR_ENOMEM (-4)
#define WMAR_EMISSING (-5) /* a required checkpoint tensor is missing      */
#define WMAR_ECALLBACK (-6) /* a wmar_logits_hook returned non-zero: the run was stopped */

/* enum values of wmar.watermarking.gentime_watermark.SeedStrategy / SplitStrategy (:95-106) */
#define WMAR_SEED_FIXED 0
#define WMAR_SEED_LINEAR 1
#define WMAR_SEED_SPATIAL 2
#define WMAR_SPLIT_RAND 0
#define WMAR_SPLIT_STRATIFIED 1

const char* wmar_last_error(void);
int wmar_version(void);

/* ---------------------------------------------------------------- watermark key
 * The greenlist of a context is a pure function of seed32 = (salt*sum(ctx)) mod 2^32
 * (GentimeWatermark._get_greenlist_ids_for_context, gentime_watermark.py:219-226, and
 * _split_with_seed :161-174).  The whole key is therefore a table of bitmaps:
 * row r = greenlist of context sum r, `vocab` bits packed LSB-first into uint32
 * words, row stride = wmar_key_row_words(vocab). */
typedef struct wmar_key_params {
    uint64_t salt_key;        /* GentimeWatermark.salt_key (default 15485863)            */
    const int64_t* alive_ids; /* host, in the order init_alivecodes produced them        */
    int64_t n_alive;
    const int64_t* dead_ids;  /* host                                                    */
    int64_t n_dead;
    int64_t vocab_size;
    double gamma;
    int32_t split_strategy;   /* WMAR_SPLIT_*  (clustering is out of scope)              */
    int32_t seed_strategy;    /* WMAR_SEED_*                                             */
} wmar_key_params;

int64_t wmar_key_row_words(int64_t vocab_size);
/* Number of table rows needed so that every reachable context sum has a row:
 * FIXED -> 1; LINEAR / SPATIAL with context size h and token ids < max_token -> h*(max_token-1)+1. */
int64_t wmar_key_table_rows(int32_t seed_strategy, int32_t context_size, int64_t max_token);
/* Host builder (MT19937 + Fisher-Yates, `n_threads` host threads; 0 = all cores).
 * Writes rows [row0, row0+n_rows) to `out_host`.  Replaces the per-row, per-step
 * _split_with_seed calls of gentime_watermark.py:266 and :281. */
int wmar_key_table_build(const wmar_key_params* key, int64_t row0, int64_t n_rows, uint32_t* out_host,
                         int32_t n_threads);
/* One greenlist in the reference's order (ids as _split_with_seed returns them). Host. */
int64_t wmar_key_greenlist(const wmar_key_params* key, uint64_t seed, int64_t* out_ids_host);

/* What every device-side watermark call needs to find a row's bitmap. */
typedef struct wmar_wm_ctx {
    const uint32_t* table_dev; /* [n_rows, row_words]                                     */
    int64_t n_rows;
    int64_t vocab_size;
    int32_t seed_strategy;
    int32_t context_size;      /* h                                                       */
    int32_t spatial_dim;       /* 16 Taming/RAR, 32 Chameleon (gentime_watermark.py:153)  */
    float delta;
} wmar_wm_ctx;

/* GentimeWatermark._process_logits (gentime_watermark.py:229-271): logits[b, G(ctx_b)] += delta,
 * in place.  past_ids_dev: int64 [B, t] with row stride `past_stride`.  Rows whose context is
 * too short are left untouched (the reference swallows the ValueError). */
int wmar_wm_process_logits(const wmar_wm_ctx* wm, float* logits_dev, int64_t B, const int64_t* past_ids_dev,
                           int64_t t, int64_t past_stride, void* stream);

/* The sampling stage of sample_with_past (mingpt.py:348-363) fused into one kernel per row:
 * watermark bias -> /temperature -> top-k -> top-p -> softmax -> argmax(p / q).
 * wm == NULL: no watermark.  top_k <= 0: off.  top_p < 0: off.  q_dev: the Exp(1) noise
 * torch.multinomial would draw, [B, V].  scratch_dev: float [B, V].  tok_out_dev: int64 [B].
 * The arithmetic is the one pinned in include/wmar_math.h. */
int wmar_sample_fused(const wmar_wm_ctx* wm, const float* logits_dev, int64_t B, int64_t V,
                      const int64_t* past_ids_dev, int64_t t, int64_t past_stride, float temperature,
                      int32_t top_k, double top_p, const float* q_dev, float* scratch_dev,
                      int64_t* tok_out_dev, void* stream);

/* GentimeWatermark.detect (gentime_watermark.py:285-344): per row of codes_dev int64 [B, L]:
 * unique (h+1)-grams -> n_scored, n_green -> p = I_gamma(n_green, 1+n_scored-n_green) in fp64
 * (NaN when n_green == 0, as scipy.special.betainc).  mask_dev (nullable): int8 [B, mask_stride],
 * entry i: -1 for the first h positions and for repeated n-grams, else the green bit.
 * Returns WMAR_ESHORT when L - h < 1 (the reference raises ValueError). */
int wmar_detect(const wmar_wm_ctx* wm, double gamma, const int64_t* codes_dev, int64_t B, int64_t L,
                int32_t* n_scored_dev, int32_t* n_green_dev, double* pval_dev, int8_t* mask_dev,
                int64_t mask_stride, void* stream);
/* number of n-grams the detector enumerates for a passage of length L (mask length = h + this) */
int64_t wmar_detect_num_ngrams(int32_t seed_strategy, int32_t context_size, int64_t L);

/* ------------------------------------------------------------------------ GPT
 * minGPT decoder with a static KV cache (deps/taming/modules/transformer/mingpt.py:125-214).
 * Tensors are looked up by their checkpoint key names relative to `transformer.`
 * (tok_emb.weight, pos_emb, blocks.N.{ln1,ln2}.{weight,bias}, blocks.N.attn.{key,query,value,proj}.{weight,bias},
 *  blocks.N.mlp.{0,2}.{weight,bias}, ln_f.{weight,bias}, head.weight), all fp32 device pointers in
 * torch's nn.Linear layout; they are repacked into MFMA-fragment order at create time and
 * need not outlive the call. */
typedef struct wmar_gpt_config {
    int32_t vocab_size, block_size, n_layer, n_head, n_embd;
    int32_t max_batch; /* KV cache and workspaces are sized for this */
} wmar_gpt_config;

typedef struct wmar_gpt wmar_gpt;

int wmar_gpt_create(const wmar_gpt_config* cfg, const char* const* names, const void* const* tensors_dev,
                    int32_t n_tensors, void* stream, wmar_gpt** out);
/* The same with creation-time options (a bit set; 0 = exactly wmar_gpt_create -- wmar_gpt_config keeps its layout, so the options
 * travel beside it).  Unknown bits: WMAR_EINVAL.  An option is fixed for the engine's life, so every captured graph of the engine
 * was captured under it.
 *   WMAR_GPT_OPT_FC2X   steps of 33..64 rows whose QKV launch is the fused k_qkvx_bx, on n_embd a multiple of 384: FC2 runs as k_fc2x
 *                       (24-column tiles x one 32-row tile x half of K: equal workgroups, TWO uniform slabs instead of 5 / 6) and the
 *                       next block's QKV launch (k_qkvx_bx<2>) and RESID_OUT fold two slabs.  Same products, another summation
 *                       order of FC2's K.  Costs a second packing of mlp.2.weight, 16 n_embd^2 bytes per block (37.7 MB at 1536;
 *                       counted by wmar_gpt_device_bytes), allocated only with the option.  Other row counts and ineligible shapes
 *                       keep the default plan; wmar_gpt_plan_info / wmar_gpt_probe_plan report what runs (S_fc2=2 fc2_hi=0,
 *                       fc2=k_fc2x, qkv=k_qkvx_bx<2>). */
#define WMAR_GPT_OPT_FC2X 1u
int wmar_gpt_create_opt(const wmar_gpt_config* cfg, uint32_t options, const char* const* names, const void* const* tensors_dev,
                        int32_t n_tensors, void* stream, wmar_gpt** out);
void wmar_gpt_destroy(wmar_gpt* g);
int64_t wmar_gpt_device_bytes(const wmar_gpt* g);

/* GPT.forward_with_past for one new token per sequence (mingpt.py:183-214): consumes
 * tok_dev int64 [B] at position `pos` (= past_length), appends K/V at `pos`, writes
 * logits_dev float [B, vocab].  Positions must be fed in order 0,1,2,... */
int wmar_gpt_decode_step(wmar_gpt* g, const int64_t* tok_dev, int64_t B, int32_t pos, float* logits_dev,
                         void* stream);

/* sample_with_past (mingpt.py:326-368) as `steps` replays of ONE captured hipGraph
 * (decode step + fused watermark/sampling + position advance; the position lives in
 * device memory).  cond_dev int64 [B] (the class token), q_dev float [steps, B, V] (noise for
 * every step, see wmar_sample_fused), tokens_out_dev int64 [B, steps].
 * logits_trace_dev (nullable): float [steps, B, V], raw model logits per step.
 * Everything is ordered on `stream`; one generate per engine at a time.  Asynchronous on the two-launch path; while the fused
 * projection launch is in use the call waits for its replays and verifies the in-launch barrier (see wmar_gpt_check). */
typedef struct wmar_sample_params {
    float temperature;
    int32_t top_k;  /* <= 0: off */
    double top_p;   /* < 0: off  */
    int32_t use_graph; /* 1: hipGraph replay, 0: eager launches */
} wmar_sample_params;

int wmar_gpt_generate(wmar_gpt* g, const wmar_wm_ctx* wm, const wmar_sample_params* sp, const int64_t* cond_dev,
                      int64_t B, int32_t steps, const float* q_dev, int64_t* tokens_out_dev,
                      float* logits_trace_dev, void* stream);

/* ------------------------------------------------------------------------ hooked generation
 * The reference's loops hand the logits of every step to an arbitrary `logit_processor` (mingpt.py:348-350, rar.py:450-451,
 * generation.py:86).  The *_hooked entry points below run the same captured step as their fused siblings, cut in two where the
 * reference calls the processor:
 *   graph A   the model step (+ wmar_cfg_mix where the model runs under guidance) -> logits_io_dev float [B, V]
 *   hook      hook(user, step, t) on the calling thread; everything it enqueues on `stream` is ordered between the two graphs;
 *             t = valid columns of past_io_dev int64 [B, past_stride].  No host synchronisation.
 *   graph B   k_sample_fused without watermark on logits_io_dev; token -> past_io_dev[:, t] and tokens_out_dev[:, step]; counters + 1
 * Both buffers are the caller's.  A non-zero return of the hook stops the run: WMAR_ECALLBACK, the engine stays usable.  The
 * in-launch barrier check is made once behind the last step (as in the fused calls): a run that raised the flag is repeated, and
 * the hook is then called again from step 0 -- it must be a function of its arguments.  The graphs of this mode live in slots of
 * their own: alternating fused and hooked calls re-captures neither. */
typedef int (*wmar_logits_hook)(void* user, int32_t step, int64_t t);

/* Guidance as a launch of its own (inside the fused sampler otherwise), fp32 [B, V] -> out_dev [B, V]; the arithmetic is the fused
 * sampler's, operation for operation:
 *   img_dev == NULL:  out = uncond + (cond - uncond) * scale_dev[step_dev ? *step_dev : 0]          (rar.py:437-442)
 *   else:             out = uncond + g_image * (img - uncond) + g_text * (cond - img)               (logits_processor.py:312-336)
 * 16-byte vector accesses when V % 4 == 0 and the four pointers are 16-byte aligned, scalar otherwise.  V <= 65536 is what the
 * engines use; any V < 2^31 is accepted. */
int wmar_cfg_mix(const float* cond_dev, const float* img_dev, const float* uncond_dev, float* out_dev, int64_t B, int64_t V,
                 const float* scale_dev, const int32_t* step_dev, float g_text, float g_image, void* stream);

/* sample_with_past with a host processor.  past_io_dev rows: the class token, then the generated tokens (mingpt.py:329,350):
 * t = step + 1, past_stride >= steps + 1.  logits_io_dev = the raw head output. */
int wmar_gpt_generate_hooked(wmar_gpt* g, const wmar_sample_params* sp, const int64_t* cond_dev, int64_t B, int32_t steps,
                             const float* q_dev, int64_t* tokens_out_dev, float* logits_io_dev, int64_t* past_io_dev,
                             int64_t past_stride, wmar_logits_hook hook, void* user, void* stream);

/* Per-kernel-class device times of the last wmar_gpt_generate call, measured with HIP events
 * recorded on the caller's stream around every launch.  Only available for eager runs
 * (use_graph = 0) after wmar_gpt_set_timing(g, 1); used by bench.py for the roofline line.
 * Classes: */
#define WMAR_T_EMBED 0   /* token+position embedding, LN statistics            */
#define WMAR_T_QKV 1     /* LN1 -> QKV GEMM -> KV cache                         */
#define WMAR_T_ATTN 2    /* decode attention                                   */
#define WMAR_T_PROJ 3    /* attention output projection (split-K slabs)        */
#define WMAR_T_RESID 4   /* residual fold + LN statistics                      */
#define WMAR_T_FC1 5     /* LN2 -> FC1 GEMM -> GELU                             */
#define WMAR_T_FC2 6     /* FC2 GEMM (split-K slabs)                           */
#define WMAR_T_HEAD 7    /* ln_f -> vocabulary head GEMM                       */
#define WMAR_T_SAMPLE 8  /* fused watermark + sampling                         */
#define WMAR_T_NCLASS 9
/* In-launch synchronisation (no reference counterpart).  At batches of 33..64 rows the output projection, its split-K reduction,
 * the residual fold and the LayerNorm statistics run as ONE launch (k_bx_xr) behind an XCD-local barrier.  wmar_gpt_create enables it
 * only when blocks with equal blockIdx % 8 share an XCD and the device holds the whole grid at once (WMAR_NO_XR=1 at creation keeps
 * the two-launch path: k_bx + k_resid_stats).  Every wait is bounded; a wait that gives up, or a block on a foreign XCD, raises a
 * device flag, later waits leave at once, and wmar_gpt_generate / wmar_gpt_decode_step -- which wait for the stream and read the
 * flags while the fused launch is in use -- switch the engine to the two-launch path and RE-RUN the call (same inputs: same
 * results; wmar_gpt_plan_info reports `barrier_fallbacks`).  On the two-launch path both calls are asynchronous again.
 * wmar_gpt_check does the same flag test for callers that enqueue single roles (wmar_gpt_profile_role): WMAR_EHIP = the launches
 * since the last check are invalid, the engine continues on the two-launch path.  WMAR_INJECT_SYNC_FAIL=1 at creation (tests)
 * raises the flag in front of the first fused call. */
int wmar_gpt_check(wmar_gpt* g, void* stream);
/* Captured graphs: how many graph slots the engine has captured AND instantiated since its creation, for the fused loop
 * (wmar_gpt_generate) and the hooked one (wmar_gpt_generate_hooked).  A call that reuses the graphs of an earlier call leaves both
 * counts as they were; a call that captures adds one per slot it fills.  Read-only, host arithmetic; either pointer may be null.
 * wmar_rar_graph_counts and wmar_cham_graph_counts are the same for those engines. */
int wmar_gpt_graph_counts(const wmar_gpt* g, int64_t* fused, int64_t* hooked);
int wmar_gpt_set_timing(wmar_gpt* g, int32_t enabled);
/* Decode attention runs 1 / 2 / 4 waves per (sequence, head) while the cache holds <= one_wave_upto / <= two_waves_upto /
 * more rows (one captured step graph per phase).  Defaults were measured at batch 64 on MI355X; a tuning entry point only --
 * results do not depend on it beyond fp32 summation order across waves.  (-1, -1) returns to the automatic schedule (one wave at
 * every length for batch x heads >= 512, 2 / 4 waves up to / beyond 128 cached rows below that). */
int wmar_gpt_set_attention_phases(wmar_gpt* g, int32_t one_wave_upto, int32_t two_waves_upto);
/* Replays ONE role's kernel `iters` times back to back on `stream` (cycling through the layers, so
 * weights stream from HBM as in a real step) between two HIP events: *avg_us = average per launch,
 * launch boundary included.  kv_len = cached rows the attention role reads. */
int wmar_gpt_profile_role(wmar_gpt* g, int32_t role, int64_t B, int32_t kv_len, int32_t iters, void* stream,
                          double* avg_us);
/* The kernels a decode step of B rows launches per role, as `role=kernel;...` text (bench.py names what it measured from this, not
 * from a table of its own).  Returns WMAR_EINVAL if buf is too small. */
int wmar_gpt_plan_info(wmar_gpt* g, int64_t B, char* buf, int64_t buf_len);
/* total_us[c], calls[c] for each class; *step_ms = average wall time of one decode step (any mode). */
int wmar_gpt_get_timing(wmar_gpt* g, double* total_us, int64_t* calls, double* step_ms);

/* Test-only stage access to a live engine (no engine path calls these; tests/test_gpu_gpt_kernels.py holds the launches of a decode
 * step to a float64 reference one at a time).  A decode step IS the sequence of stages below, one launch each; the engine walks it,
 * the probe runs parts of it.  Matrix-core plan (13..128 rows, or any row count on an engine without the small-batch weights):
 *   EMBED       k_resid_stats<embed>     x = tok_emb[tok] + pos_emb[pos] (packed fp32), stats = per-chunk (sum, sum of squares) in fp64
 *   RESID_IN    k_resid_stats            layer > 0 and QKV does not fold (S_qx == 0): x += bfc2[l-1] + (FC2 slabs of layer l-1), stats
 *   QKV         k_qkvx / k_qkvx_bx       (S_qx > 0) x' = x + bfc2[l-1] + slabs into the OTHER of x / x2 (layer 0: a copy), stats_q, and the
 *                                        K slices of (Wqkv * ln1.weight) x' into qkv_slabs;  or k_gemm<EPI_PACKED> (S_qkv pieces of x)
 *   ATTN        k_attn_decode<HD,NW>     LN1 algebra + bias on the summed pieces, K / V row appended at pos, softmax(q K^T) V -> y (and yq)
 *   PROJ        k_gemm / k_bx / k_bx_xr  slabs = K slices of Wproj y; k_bx_xr also folds them: x += bproj + slabs, stats (16 chunks)
 *   RESID_ATTN  k_resid_stats            x += bproj + slabs, stats                          (absent behind k_bx_xr)
 *   FC1         k_fc1x / k_gemm<GELU>    hbuf = gelu(LN2 algebra on (Wfc1 * ln2.weight) x + bfc1)
 *   FC2         k_gemm<EPI_PACKED>       slabs = S_fc2 K slices of Wfc2 hbuf (+ 1 for the first fc2_hi column tiles);  or k_fc2x
 *                                        (WMAR_GPT_OPT_FC2X): slab s = K half s of Wfc2 hbuf, S_fc2 = 2, fc2_hi = 0
 *   RESID_OUT   k_resid_stats            behind the last layer: x += bfc2[L-1] + slabs, stats
 *   HEAD        k_gemm<EPI_LOGITS,LN>    logits = ln_f algebra on (Whead * ln_f.weight) x + bhead
 * Small-batch plan (1..12 rows, n_embd 1536, head_dim 64): EMBED k_sembed, QKV / PROJ / FC1 / FC2 / HEAD k_sgemv<..>, ATTN k_sattn on
 * the row-major xs / qs / ys / hs; PROJ and FC2 add the residual in place, so there is no RESID_* stage.
 * wmar_gpt_probe_run sets the position, runs stages first_stage..last_stage of block `layer` (EMBED, RESID_OUT and HEAD ignore it) with
 * the engine's own StepPlan, buffers and attention phase for (B, pos + 1 cached rows), and waits for the stream.  first_stage and
 * last_stage must exist in the plan for B (WMAR_EINVAL otherwise); absent stages between them are passed over as the step does.
 * The residual stream buffer a stage reads follows the step: with S_qx > 0 it is x in front of an even layer's QKV and x2 behind
 * it (odd layers the other way round), RESID_OUT and HEAD read what block n_layer - 1 left; otherwise always x.  A raised in-launch
 * barrier flag is reported as WMAR_EHIP (the stages run are invalid; the engine continues on the two-launch path, as after
 * wmar_gpt_check).
 * wmar_gpt_probe_copy, wmar_rar_probe_copy and wmar_cham_probe_copy share one contract (stated here once): the call copies device to
 * device between ptr_dev and the engine buffer `name` of block `layer` (to_engine != 0: into the engine, else out of it) and waits
 * for the stream.  It returns the buffer's size in bytes, or a negative status: WMAR_EINVAL for a name the engine does not know, for
 * a buffer this engine does not have (its shape is not eligible for the kernel that uses it) and for a `bytes` other than exactly
 * that size; WMAR_EHIP when the copy fails.  With ptr_dev null nothing is copied and `bytes` is ignored: a size query.
 * The buffers of wmar_gpt_probe_copy: packed buffers are laid out for the MT of the step that wrote them (MT = 1 / 2 / 4 row tiles for B <= 32 / 64 / 128), sizes are
 * for Mpad = 32 * MT(max_batch) rows:
 *   x, x2, y [D/8][MT][64][4] fp32; hbuf [4D/8][MT][64][4]; yq [D/16][2][3][64][4] u32 (bf16 planes, 64-row engines only);
 *   slabs [8] pieces of D columns, qkv_slabs [8] pieces of 3D columns (piece stride = D resp. 3D x 32 MT floats of the step's MT);
 *   stats [64][Mpad][2] fp64, stats_q [32][Mpad][2] fp64 (chunk stride = 32 MT rows of the step's MT);
 *   kcache, vcache [max_batch][H][block_size][head_dim] fp32 of block `layer`; xs, ys, qs [12][D], hs [12][4D] row-major fp32;
 *   wqkv, wqkvx_bx, wproj, wproj_bx, wfc1, wfc1x16, wfc1x8, wfc2, wfc2x16, wfc2x8, bqkv, cqkv, bproj, bfc1, cfc1, bfc2 of block `layer`;
 *   whead, bhead, chead.
 * wmar_gpt_probe_plan writes, for a step of B rows attending to kv_len cached rows,
 *   "small=0 MT=.. S_qx=.. nkeep=.. S_qkv=.. S_proj=.. S_fc2=.. fc2_hi=.. nch=.. nch_ln2=.. pingpong=.. x_head=x|x2 attn_waves=..
 *    rowmajor=.. proj=gemm|bx|bx_xr head=ntw2|N,PER fc1_tiles=.. head_tiles=.. xcd_ok=.. xr_eligible=.. barrier_fallbacks=..
 *    stages=EMBED,QKV,.. kernels=<the text of wmar_gpt_plan_info>"
 * (stages: those of block 1 when n_layer > 1, else block 0; head=N,PER: N launches of at most PER column tiles; fc1_tiles / head_tiles:
 * row tiles per workgroup of the k_gemm that runs FC1 / the head, 0 where another kernel does; xcd_ok: the block -> XCD grouping and
 * residency as measured at creation, a property of the device; xr_eligible: shape and switches admit k_bx_xr, so proj is bx_xr
 * exactly when both are 1 and no barrier has fallen back). */
enum {
    WMAR_GPT_STAGE_EMBED = 0, WMAR_GPT_STAGE_RESID_IN, WMAR_GPT_STAGE_QKV, WMAR_GPT_STAGE_ATTN, WMAR_GPT_STAGE_PROJ,
    WMAR_GPT_STAGE_RESID_ATTN, WMAR_GPT_STAGE_FC1, WMAR_GPT_STAGE_FC2, WMAR_GPT_STAGE_RESID_OUT, WMAR_GPT_STAGE_HEAD
};
int wmar_gpt_probe_run(wmar_gpt* g, const int64_t* tok_dev, int64_t B, int32_t pos, int32_t layer, int32_t first_stage,
                       int32_t last_stage, float* logits_dev, void* stream);
int64_t wmar_gpt_probe_copy(wmar_gpt* g, const char* name, int32_t layer, void* ptr_dev, int64_t bytes, int32_t to_engine,
                            void* stream);
int wmar_gpt_probe_plan(wmar_gpt* g, int64_t B, int32_t kv_len, char* buf, int64_t buf_len);

/* ------------------------------------------------------------------------ RAR
 * RAR generator (deps/rar/modeling/rar.py): adaLN blocks, per-head q/k LayerNorm, KV cache,
 * classifier-free guidance.  Tensors by the checkpoint's key names (cls_token, embeddings.weight,
 * pos_embed, target_aware_pos_embed, timesteps_embeddings, blocks.N.{norm1,norm2}.{weight,bias},
 * blocks.N.attn.{qkv,proj}.{weight,bias}, blocks.N.attn.{q_norm,k_norm}.{weight,bias},
 * blocks.N.mlp.{fc1,fc2}.{weight,bias}, blocks.N.adaLN_modulation.1.{weight,bias},
 * adaln_before_head.adaLN_modulation.1.{weight,bias}, lm_head.{weight,bias}). */
typedef struct wmar_rar_config {
    int32_t hidden_size, num_hidden_layers, num_attention_heads, intermediate_size;
    int32_t image_seq_len, codebook_size, condition_num_classes;
    int32_t max_batch;   /* images per call; rows double under guidance */
} wmar_rar_config;

typedef struct wmar_rar wmar_rar;

int wmar_rar_create(const wmar_rar_config* cfg, const char* const* names, const void* const* tensors_dev,
                    int32_t n_tensors, void* stream, wmar_rar** out);
void wmar_rar_destroy(wmar_rar* g);
int64_t wmar_rar_device_bytes(const wmar_rar* g);

/* RAR.forward_fn for ONE sequence position with a warm KV cache (rar.py:319-405): row m consumes
 * tok_dev[m] (-1 = the cls token) at position `pos` under condition id cond_ids_dev[m] (already offset:
 * class + codebook_size + 1, or the "none" id) and yields logits_dev float [M, codebook].  Positions in
 * order 0,1,2,...  Used by the parity tests. */
int wmar_rar_forward_position(wmar_rar* g, const int64_t* tok_dev, const int64_t* cond_ids_dev, int64_t M, int32_t pos,
                              float* logits_dev, void* stream);

/* RAR.generate (rar.py:408-459): class_ids_dev int64 [B] in [0, classes); cfg_scale_host float
 * [image_seq_len] = the reference's per-step cfg_scale (host; ignored when use_guidance == 0);
 * q_dev float [image_seq_len, B, V] Exp(1) noise; tokens_out_dev int64 [B, image_seq_len].
 * The watermark context is the generated ids only, so the first token is never biased. */
int wmar_rar_generate(wmar_rar* g, const wmar_wm_ctx* wm, const int64_t* class_ids_dev, int64_t B,
                      const float* cfg_scale_host, int32_t use_guidance, float temperature, const float* q_dev,
                      int64_t* tokens_out_dev, int32_t use_graph, void* stream);

/* RAR.generate with a host processor (see "hooked generation" above).  past_io_dev rows: the generated tokens only, t = step
 * (empty at the first step, rar.py:420,451), past_stride >= image_seq_len.  logits_io_dev = after guidance, before temperature. */
int wmar_rar_generate_hooked(wmar_rar* g, const int64_t* class_ids_dev, int64_t B, const float* cfg_scale_host,
                             int32_t use_guidance, float temperature, const float* q_dev, int64_t* tokens_out_dev,
                             int32_t use_graph, float* logits_io_dev, int64_t* past_io_dev, int64_t past_stride,
                             wmar_logits_hook hook, void* user, void* stream);

/* RAR generation with the Gumbel-key sampler below instead of multinomial + greenlist (BASELINE
 * config "RAR-XL ... Gumbel-key watermark"; an EXTENSION -- the reference image code has no such
 * path).  log_rs_dev float [V]: the fixed key (wmar_gumbel_key_build). */
int wmar_rar_generate_gumbel(wmar_rar* g, const int64_t* class_ids_dev, int64_t B, const float* cfg_scale_host,
                             int32_t use_guidance, float temperature, float top_p, int32_t top_k,
                             const float* log_rs_dev, int64_t* tokens_out_dev, int32_t use_graph, void* stream);

/* The same with a CONTEXT-KEYED key (ngram in 1..WMAR_MAX_CONTEXT).  Context = the generated ids only.  Position l >= ngram of row b
 * is sampled with the key of hash = h0 ^ ids[b, l-ngram] ^ ... ^ ids[b, l-1], derived on the device inside the step (the arrays of
 * wmar_gumbel_key_rows); h0 = the hash of the empty window (first randint(0, 2^31 - 1) of the CPU generator seeded with the
 * watermark seed: the caller computes it).  Positions l < ngram are unkeyed: u_dev float [ngram, B, V], uniform in [0, 1), takes the
 * place of rs in the same sampler arithmetic -- plain sampling from p.  One captured graph serves every position (keyed or not is
 * decided on the device-side step counter); use_graph = 0 gives the same tokens. */
int wmar_rar_generate_gumbel_ctx(wmar_rar* g, const int64_t* class_ids_dev, int64_t B, const float* cfg_scale_host,
                                 int32_t use_guidance, float temperature, float top_p, int32_t top_k, uint64_t h0, int32_t ngram,
                                 const float* u_dev, int64_t* tokens_out_dev, int32_t use_graph, void* stream);

/* In-launch synchronisation of the RAR engine: the fused residual + adaLN modulation launch of a block (k_resid_mod) lets its
 * workgroups wait for each other's partial sums.  wmar_rar_create enables it when the device holds the whole grid at once
 * (occupancy x compute units; WMAR_NO_XR=1 disables it), otherwise the same work runs as a two-launch pair (bit-identical results).
 * A wait that gives up raises a device flag; wmar_rar_generate* / wmar_rar_forward_position wait for the stream while the fused
 * launch is in use, and on a raised flag switch to the two-launch pair and RE-RUN the call.  wmar_rar_check: the same flag test
 * for other callers (WMAR_EHIP = the launches since the last check are invalid).  wmar_rar_launch_status: whether the fused
 * launch is still in use, and how many calls were re-run. */
int wmar_rar_launch_status(const wmar_rar* g, int32_t* fused, int32_t* fallbacks);
int wmar_rar_check(wmar_rar* g, void* stream);
int wmar_rar_graph_counts(const wmar_rar* g, int64_t* fused, int64_t* hooked);      /* see wmar_gpt_graph_counts */

/* Test-only stage access to a live engine (no engine path calls these; tests/test_gpu_rar_kernels.py holds the launches of a RAR
 * position to a float64 reference one at a time).  A position IS the sequence of stages below, one launch each (RESID_* on the
 * two-launch pair: two); the engine walks it, the probe runs parts of it.  M rows, MT = 1 / 2 / 4 row tiles for M <= 32 / 64 / 128;
 * MTc = row tiles of the adaLN rows (MT, or those of Bhalf under shared_u); bx = the 128-row plan on the bf16 matrix pipe.
 *   EMBED       k_rar_embed             x = token vector + pos_embed[p] (+ target_aware_pos_embed[p + 1] for p >= 1), stats; sc (and scq
 *                                       planes where ADALN runs as k_bx) = SiLU(emb[cond] + timesteps[p]) of the first 32 MTc rows.
 *                                       tok_dev given: row m takes tok_dev[m] (-1 = cls); null: p = 0 cls, p = 1 emb[cond[m]],
 *                                       p >= 2 emb[ids[(m % Bhalf) * image_seq_len + p - 2]]
 *   ADALN       k_gemm<EPI_PACKED> / k_bx<4,20,2>   mod = sc Wada^T + bada, packed [Ntot/8][MTc][64][4]
 *   MOD_IN      k_modulate              h (bx: xq planes) = LayerNorm(x; norm1 of block 0, eps 1e-6) (1 + scale) + shift
 *   QKV         k_gemm<EPI_PACKED> / k_bx<2,PER,4>  qkv_slabs = S_qkv K slices of Wqkv h (head_dim 80 on bx: row-major pieces)
 *   ATTN        k_attn_decode<HD,1,1> / k_attn_decode80<1>   bias, q_norm / k_norm per head (eps 1e-6), K / V row appended at p,
 *                                       softmax(q K^T / sqrt(hd)) V -> y (bx: yq planes)
 *   PROJ        k_gemm / k_bx<1,PER,4>  slabs = S_proj K slices of Wproj y
 *   RESID_ATTN  k_resid_mod (site 2l)   x += gate_msa (bproj + slabs); h = LayerNorm(x; norm2) (1 + scale_mlp) + shift_mlp; part
 *   FC1         k_gemm<EPI_GELU> / k_bx<1,10,4,GELU,8,XF>   hbuf (bx: hq planes) = gelu(Wfc1 h + bfc1)
 *   FC2         k_gemm / k_bx<2,PER,4>  slabs = S_fc2 K slices of Wfc2 hbuf
 *   RESID_MLP   k_resid_mod (site 2l+1) x += gate_mlp (bfc2 + slabs); h (bx: xq) = block l + 1's norm1 modulation, or behind the last
 *                                       block the final layer's affine-free norm (its adaLN columns: scale first, then shift) into h
 *   HEAD        k_gemm<EPI_LOGITS>      logits = Whead h + bhead
 * Rows at or past Bhalf under shared_u take shift / scale / gate from row p of the row-major table mod_u [T][Ntot] instead of mod.
 * adaLN columns: block l at 6 D l: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp; the final layer at 6 D L: scale, shift.
 * wmar_rar_probe_run copies cond_ids_dev (int64 [M], may be null behind EMBED) into the engine, sets the position, builds the
 * unconditional table if shared_u != 0 and it is not ready (M must then be 2 Bhalf; otherwise Bhalf = M), poisons the `part` sites of the
 * RESID_* stages it runs as a position does, runs stages first_stage..last_stage of block `layer` (EMBED, ADALN, MOD_IN and HEAD
 * ignore it) with the engine's own RarPlan and buffers, and waits for the stream.  tok_dev null selects the generate form of the
 * embedding, reading the engine's `ids`.  A raised in-launch wait flag is reported as WMAR_EHIP, not re-run (the stages run are
 * invalid; the engine continues on the two-launch pair, as after wmar_rar_check).
 * The buffers of wmar_rar_probe_copy (its contract: at wmar_gpt_probe_copy above): packed buffers are laid out for the MT of the position that wrote them, sizes are for Mpad = 32 MT(2 max_batch) rows:
 *   x, h, y, sc [D/8][MT][64][4] fp32 (sc: MTc row tiles); hbuf [F/8][MT][64][4]; mod [Ntot/8][MTc][64][4]; mod_u [32 ceil(T/32)][Ntot];
 *   slabs [8] pieces of D columns, qkv_slabs [S_qkv of the bx plan, else 1] pieces of 3 D columns (piece stride = columns x 32 MT floats);
 *   xq, yq [D/16][MT][3][64][4] u32 and hq [F/16][MT][3][64][4] (bf16 planes, engines with the bx plan), scq [D/16][2][3][64][4];
 *   stats [64][Mpad][2] fp64 (chunk stride 32 MT rows); part [2 L sites][nrm][32 MT][2] u64, sites packed at the position's MT;
 *   logits [2 max_batch][V]; ids int64 [max_batch][image_seq_len]; cond_ids int64 [2 max_batch]; ctr int32 [4] (pos, step, len);
 *   kcache, vcache [2 max_batch][H][image_seq_len + 2][head_dim] fp32 of block `layer`;
 *   wqkv, wproj, wfc1, wfc2 (k_pack_linear order), wqkv_bx, wproj_bx, wfc1_bx, wfc2_bx (k_pack_bx order), bqkv, bproj, bfc1, bfc2,
 *   norm1_w, norm1_b, norm2_w, norm2_b, q_norm_w, q_norm_b, k_norm_w, k_norm_b of block `layer`; wada, wada_bx, bada, whead, bhead.
 * wmar_rar_probe_plan writes, for a position of M rows attending to kv_len cached rows,
 *   "MT=.. MTc=.. bx=.. ada_bx=.. fc1_bx=.. rowmajor=.. S_qkv=.. S_proj=.. S_fc2=.. PER_qkv=.. PER_proj=.. PER_fc2=.. nch=.. nrm=.. kpw=..
 *    fused=.. fallbacks=.. ada_tiles=.. fc1_tiles=.. head_tiles=.. attn_waves=.. stages=EMBED,ADALN,.. kernels=embed=..;adaln=..;.."
 * (nch: statistics chunks of EMBED / MOD_IN; nrm, kpw: chunks and k-blocks per wave of k_resid_mod; *_tiles: row tiles per workgroup
 * of the k_gemm that runs the adaLN GEMM / FC1 / the head, 0 where k_bx does; PER_*: 0 off the bx plan; kernels: the instantiation
 * behind every stage).  Every figure comes from the helper the launch itself uses. */
enum {
    WMAR_RAR_STAGE_EMBED = 0, WMAR_RAR_STAGE_ADALN, WMAR_RAR_STAGE_MOD_IN, WMAR_RAR_STAGE_QKV, WMAR_RAR_STAGE_ATTN, WMAR_RAR_STAGE_PROJ,
    WMAR_RAR_STAGE_RESID_ATTN, WMAR_RAR_STAGE_FC1, WMAR_RAR_STAGE_FC2, WMAR_RAR_STAGE_RESID_MLP, WMAR_RAR_STAGE_HEAD
};
int wmar_rar_probe_run(wmar_rar* g, const int64_t* tok_dev, const int64_t* cond_ids_dev, int64_t M, int64_t Bhalf, int32_t shared_u,
                       int32_t pos, int32_t layer, int32_t first_stage, int32_t last_stage, float* logits_dev, void* stream);
int64_t wmar_rar_probe_copy(wmar_rar* g, const char* name, int32_t layer, void* ptr_dev, int64_t bytes, int32_t to_engine,
                            void* stream);
int wmar_rar_probe_plan(wmar_rar* g, int64_t M, int64_t Bhalf, int32_t shared_u, int32_t kv_len, char* buf, int64_t buf_len);

/* ----------------------------------------------------------------- Gumbel key (row G1)
 * Aaronson-style sampling of wmar_audio/watermark/engine.py:29-75 (`gumbel_sample`) and its
 * detector :123-134 (`gumbel_score_tok`).  The key of a row is rs = torch.rand(V, generator =
 * CPU MT19937 seeded with the row's window hash) (engine.py:64-66); with ngram = 0 the hash is
 * the seed itself (:17-18), so one key serves every row.
 *
 * wmar_gumbel_key_build (host): rs_host[v] = (mt.next() & 0xffffff) * 2^-24 (torch's fp32
 * uniform), log_rs_host[v] = (float)log(rs) and score_host[v] = (float)-log(1 - rs).  Any output
 * may be null. */
int wmar_gumbel_key_build(uint64_t seed, int64_t vocab_size, float* rs_host, float* log_rs_host, float* score_host);

/* next_token[b] = argmax_v rs[v]^(1/p[v]) with p = softmax(logits/temp) after the optional top-p
 * (descending sort, drop where cumsum - p > top_p, renormalise) or else top-k (others := 1e-6,
 * renormalise) -- engine.py:41-75.  The race is run as argmax log(rs[v]) * (1/p[v]) (monotone
 * image; scores below log(2^-150) collapse to one class like the reference's fp32 underflow).
 * use_sampling == 0 or temp <= 0: plain argmax(logits).  key_row_stride: elements between the
 * keys of consecutive rows (0: one shared key).  V <= 16384. */
int wmar_gumbel_sample(const float* logits_dev, int64_t B, int64_t V, const float* log_rs_dev, int64_t key_row_stride,
                       int32_t use_sampling, float temp, float top_p, int32_t top_k, int64_t* tok_out_dev, void* stream);

/* Probe (tests, debugging): one launch of the same sampler with the argument set the decode loop gives it (wmar_rar_generate_gumbel).
 * logits_uncond_dev (nullable) float [B, V] and cfg_scale_dev float [n_steps]: the row sampled is u + (x - u) * cfg_scale[*step_dev];
 * step_dev / t_dev (nullable, device int32, read as 0 when null); the token of row b lands at tok_out_dev[b * tok_out_stride + *step_dev]
 * and, with past_append_dev, at past_append_dev[b * past_stride + *t_dev].  The call reads both counters back first and refuses
 * (WMAR_EINVAL, nothing launched) a step or length outside those rows or the scale table; it waits for the stream. */
int wmar_gumbel_probe_sample(const float* logits_dev, const float* logits_uncond_dev, const float* cfg_scale_dev, int32_t n_steps,
                             const int32_t* step_dev, const int32_t* t_dev, int64_t B, int64_t V, const float* log_rs_dev,
                             int64_t key_row_stride, int32_t use_sampling, float temp, float top_p, int32_t top_k,
                             int64_t* tok_out_dev, int64_t tok_out_stride, int64_t* past_append_dev, int64_t past_stride,
                             void* stream);

/* gumbel_score_tok for tokens int64 [B, L]: scores_f32_dev[b,l] = -log(1 - rs)[token] and
 * scores_i64_dev[b,l] = that value truncated toward zero (what the reference returns, because it
 * accumulates into zeros_like(tokens)).  Either output may be null. */
int wmar_gumbel_score(const int64_t* tokens_dev, int64_t B, int64_t L, int64_t V, const float* score_key_dev,
                      int64_t key_row_stride, int64_t* scores_i64_dev, float* scores_f32_dev, void* stream);

/* The arrays of wmar_gumbel_key_build for N window hashes, derived ON THE DEVICE (MT19937 per hash, state in LDS; the logarithms in
 * fp64, rounded once): rs / log_rs / score rows float [N, V], bit-equal to the host builder's for seed = hash & 0xffffffff.
 * hash_dev int64 [N] on the device; any output may be null.  Asynchronous: no host copy, no synchronisation. */
int wmar_gumbel_key_rows(const int64_t* hash_dev, int64_t N, int64_t V, float* rs_out_dev, float* log_rs_out_dev,
                         float* score_out_dev, void* stream);

/* Detector of the context-keyed watermark for tokens int64 [B, L], ngram in 1..WMAR_MAX_CONTEXT, V <= 16384, L <= 4096.
 * Position l >= ngram is scored when its (ngram+1)-tuple ids[b, l-ngram .. l] has not occurred at an earlier scored position of
 * the row: scored_mask_dev int8 [B, L], n_scored_dev int32 [B] (nullable), scores_f32_dev[b, l] = -log(1 - rs_hash)[ids[b, l]] with
 * hash = h0 ^ ids[b, l-ngram] ^ ... ^ ids[b, l-1] (0 where unscored).  L <= ngram: WMAR_ESHORT.  Token ids outside [0, V) are
 * rejected like wmar_gumbel_score's (the call waits for the stream). */
int wmar_gumbel_score_ctx(const int64_t* tokens_dev, int64_t B, int64_t L, int64_t V, uint64_t h0, int32_t ngram,
                          float* scores_f32_dev, int8_t* scored_mask_dev, int32_t* n_scored_dev, void* stream);

/* ------------------------------------------------------------------ Chameleon (row C1)
 * Chameleon / Anole text->image decode: deps/chameleon/inference/transformer.py:288-353
 * (Transformer), chameleon.py:299-389 (ImageDecoder), logits_processor.py:135-156, 312-336,
 * token_selector.py:26-47.  bf16 weights and activations, fp32 accumulation.  Tensors by the
 * checkpoint's key names (tok_embeddings.weight, layers.N.attention.{wqkv,wo}.weight,
 * layers.N.attention.{q,k}_normalization.{weight,bias}, layers.N.feed_forward.{w13,w2}.weight,
 * layers.N.{attention,ffn}_norm.weight, norm.weight, output.weight); all bf16 (tensors_bf16 = 1,
 * the reference's storage) or all fp32 (rounded to bf16 at pack time). */
typedef struct wmar_cham_config {
    int32_t dim, n_layers, n_heads, n_kv_heads, vocab_size;
    int32_t ffn_hidden;        /* FeedForward hidden size after the multiple_of rounding (transformer.py:175-179) */
    float norm_eps, rope_theta;
    int32_t qk_normalization;  /* LayerNorm(head_dim) on q and k (transformer.py:74-77) */
    int32_t swin_norm;         /* must be 0 (the 30B block order is not built) */
    int32_t max_rows;          /* sequences per step = 3 * images per call */
    int32_t max_seq_len;       /* prompt + generated tokens per sequence */
    int32_t tensors_bf16;
} wmar_cham_config;

typedef struct wmar_cham_sample_params {
    float temperature;
    double top_p;                                     /* < 0: off */
    float guidance_scale_text, guidance_scale_image;  /* Options.Image.cfg: 3.0 / 1.2 */
    int32_t use_graph;
    int32_t pad_id;   /* vocab.pad_id: what AlignPromptRight pads short prompts with on the left (alignment.py:27-41); the
                       * watermark context of the first image tokens can reach into it when context_size >= 2 */
} wmar_cham_sample_params;

typedef struct wmar_cham wmar_cham;

int wmar_cham_create(const wmar_cham_config* cfg, const char* const* names, const void* const* tensors_dev,
                     int32_t n_tensors, void* stream, wmar_cham** out);
void wmar_cham_destroy(wmar_cham* g);
int64_t wmar_cham_device_bytes(const wmar_cham* g);
int wmar_cham_graph_counts(const wmar_cham* g, int64_t* fused, int64_t* hooked);    /* see wmar_gpt_graph_counts */

/* One token per sequence: row m consumes tok_dev[m] at position pos_dev[m] (its KV cache must hold
 * positions 0..pos-1) -> logits_dev float [M, vocab] (nullable: cache update only).  This is
 * Transformer.forward_with_attn_bias with q_seqlen = 1 per sequence (model_adapter.py:106-113);
 * a prompt is prefilled by calling it once per position. */
int wmar_cham_forward_tokens(wmar_cham* g, const int64_t* tok_dev, const int32_t* pos_dev, int64_t M, float* logits_dev,
                             void* stream);

/* ImageDecoder (chameleon.py:299-389) for B prompts: prompt_tokens_host = the 3B token lists of
 * _split_inputs_for_cfg (:351-372; full-conditioned, image-conditioned, unconditioned) laid end to
 * end, prompt_lens_host int32 [3B].  Per generated token: guidance mix -> watermark bias ->
 * allow-only (allow_dev: bit per vocabulary entry, nullable; allow_ids_dev: the same set as ascending int32 ids
 * [n_allow], nullable -- with it the sampler works on the compacted row, which is exact) -> temperature -> top-p -> softmax ->
 * multinomial on the first stream (q_dev float [n_tokens, B, vocab] Exp(1) noise, one [B, vocab]
 * draw per token as probs.multinomial makes).  tokens_out_dev int64 [B, n_tokens] (vocabulary ids).
 * The watermark context is the whole right-aligned input row, as the reference's processors see it (generation.py:86): its
 * last 3 entries (prompt tokens, left-padded with pad_id) are kept in front of the generated tokens, enough for every linear
 * context size the library supports (<= 3).  SPATIAL seeding is rejected: the reference does not offer it for Chameleon. */
int wmar_cham_generate_image(wmar_cham* g, const wmar_wm_ctx* wm, const int64_t* prompt_tokens_host,
                             const int32_t* prompt_lens_host, int64_t B, const wmar_cham_sample_params* sp,
                             const uint32_t* allow_dev, const int32_t* allow_ids_dev, int32_t n_allow, const float* q_dev,
                             int32_t n_tokens, int64_t* tokens_out_dev, void* stream);

/* The same with a host processor (see "hooked generation" above): guidance mix (wmar_cfg_mix) -> hook -> allow-only -> temperature
 * -> top-p -> multinomial (chameleon.py:313-327).  past_io_dev rows: the first stream's whole prompt, left-padded with pad_id to the
 * longest of the 3B prompts (P entries), then the generated tokens: t = P + step, past_stride >= P + n_tokens.  The reference hands
 * its processors all 3B rows and samples from the first third (token_selector.py:34-47); here the processor sees that third only. */
int wmar_cham_generate_image_hooked(wmar_cham* g, const int64_t* prompt_tokens_host, const int32_t* prompt_lens_host, int64_t B,
                                    const wmar_cham_sample_params* sp, const uint32_t* allow_dev, const int32_t* allow_ids_dev,
                                    int32_t n_allow, const float* q_dev, int32_t n_tokens, int64_t* tokens_out_dev,
                                    float* logits_io_dev, int64_t* past_io_dev, int64_t past_stride, wmar_logits_hook hook,
                                    void* user, void* stream);

/* Test-only stage access to a live engine (no engine path calls these; tests/test_gpu_cham_kernels.py holds every launch of a
 * decode step to a float64 reference on its own).  A decode step is EMBED, then per block QKV .. RESID_FFN, then HEAD:
 *   EMBED       k_cham_resid<true>     x = tok_embeddings[tok] (packed bf16), ssq = per-64-feature sums of squares of x (fp64)
 *   QKV         k_bgemm<MT,SLAB>       big_slabs = stream-K pieces of (wqkv * attention_norm.weight) x        (fp32, no 1/rms yet)
 *   ATTN        k_cham_attn<HD,NWA>    1/rms, qk LayerNorm, RoPE, K/V row appended at pos, softmax(q K^T) V -> y (packed bf16)
 *   WO          k_bgemm<MT,SLAB>       slabs = pieces of wo y
 *   RESID_ATTN  k_cham_resid<false>    x = bf16(x + bf16(sum of the pieces in piece order)), ssq of the new x
 *   W13         k_bgemm<MT,SLAB>       big_slabs = pieces of (w13 * ffn_norm.weight) x, x1 / x3 interleaved 16 features at a time
 *   SWIGLU      k_cham_swiglu          hbuf = bf16(bf16(silu(u1)) * u3), u = bf16(1/rms * sum of pieces)     (packed bf16)
 *   W2          k_bgemm<MT,SLAB>       slabs = pieces of w2 hbuf
 *   RESID_FFN   k_cham_resid<false>    as RESID_ATTN
 *   HEAD        k_bgemm<MT,LOGITS>     logits = bf16(1/rms * (output.weight * norm.weight) x) as fp32 [M, vocab]
 * wmar_cham_probe_run runs stages first_stage..last_stage of block `layer` with the engine's own plan and buffers and waits for
 * the stream; tok_dev / pos_dev are copied in only when EMBED is among them, logits_dev is needed only for HEAD.
 * The buffers of wmar_cham_probe_copy (its contract: at wmar_gpt_probe_copy above):
 *   x, y [D/16][MT][64][8] bf16; hbuf [F/16][MT][64][8] bf16; slabs [16][D/16][MT][64][8] fp32;
 *   big_slabs [16][max(D + 2 Dkv, 2 F)/16][MT][64][8] fp32 (a piece's stride is the producing GEMM's own width);
 *   ssq [ceil(D/64)][32 MT] fp64; kcache, vcache [max_rows][Hkv][max_seq_len][head_dim] bf16 of block `layer`;
 *   rope [max_seq_len][head_dim/2] (cos, sin) fp32; wqkv, wo, w13, w2 (block `layer`), whead: packed weights [N/32][K/16][64][8] bf16.
 * wmar_cham_probe_plan writes "MT=.. sk_qkv=C,U,G sk_o=.. sk_13=.. sk_2=.. sk_head=.. kernels=k_bgemm<MT,SLAB>;k_bgemm<MT,LOGITS>;
 * k_cham_attn<HD,NWA>" for a step of M rows: the stream-K decomposition (chunks per group, units, workgroups) and the kernel
 * instantiations the dispatch launches. */
enum {
    WMAR_CHAM_STAGE_EMBED = 0, WMAR_CHAM_STAGE_QKV, WMAR_CHAM_STAGE_ATTN, WMAR_CHAM_STAGE_WO, WMAR_CHAM_STAGE_RESID_ATTN,
    WMAR_CHAM_STAGE_W13, WMAR_CHAM_STAGE_SWIGLU, WMAR_CHAM_STAGE_W2, WMAR_CHAM_STAGE_RESID_FFN, WMAR_CHAM_STAGE_HEAD
};
int wmar_cham_probe_run(wmar_cham* g, const int64_t* tok_dev, const int32_t* pos_dev, int64_t M, int32_t layer, int32_t first_stage,
                        int32_t last_stage, float* logits_dev, void* stream);
int64_t wmar_cham_probe_copy(wmar_cham* g, const char* name, int32_t layer, void* ptr_dev, int64_t bytes, int32_t to_engine,
                             void* stream);
int wmar_cham_probe_plan(wmar_cham* g, int64_t M, char* buf, int64_t buf_len);

/* The ImageDecoder logits pipeline of one step as ONE launch (chameleon.py:313-327, generation.py:84-93):
 * logits3_dev float [3B, V] = [full | image-conditioned | unconditioned] rows; guidance mix
 * (logits_processor.py:312-336) -> watermark bias (called positionally on the input rows,
 * past_ids_dev int64 [B, past_stride] with t valid entries; nullable for FIXED keys) ->
 * allow-only bitmap (nullable; allow_ids_dev / n_allow: the same set as ascending ids, enables row compaction) ->
 * /temperature -> top-p (< 0: off) -> softmax ->
 * argmax(p / q) on the first stream (token_selector.py:36-47).  tok_out_dev int64 [B]. */
int wmar_cham_sample(const wmar_wm_ctx* wm, const float* logits3_dev, int64_t B, int64_t V, const int64_t* past_ids_dev,
                     int64_t t, int64_t past_stride, float temperature, double top_p, float guidance_scale_text,
                     float guidance_scale_image, const uint32_t* allow_dev, const int32_t* allow_ids_dev, int32_t n_allow,
                     const float* q_dev, float* scratch_dev, int64_t* tok_out_dev, void* stream);

/* ---------------------------------------------------------------------- VQGAN
 * Taming VQGAN (deps/taming/models/vqgan.py:30-73, modules/diffusionmodules/model.py:343-538,
 * modules/vqvae/quantize.py:272-331).  Tensors by key name relative to `first_stage_model.`
 * (encoder.*, decoder.*, quantize.embedding.weight, quant_conv.*, post_quant_conv.*). */
typedef struct wmar_vq_config {
    int32_t ch, num_res_blocks, resolution, in_channels, out_ch, z_channels, embed_dim, n_embed;
    int32_t n_levels;
    int32_t ch_mult[8];
    int32_t n_attn_res;
    int32_t attn_resolutions[8];
    int32_t max_batch;
} wmar_vq_config;

typedef struct wmar_vq wmar_vq;

int wmar_vq_create(const wmar_vq_config* cfg, const char* const* names, const void* const* tensors_dev,
                   int32_t n_tensors, void* stream, wmar_vq** out);
void wmar_vq_destroy(wmar_vq* v);
int64_t wmar_vq_device_bytes(const wmar_vq* v);

/* TamingARMMWrapper.codes_to_images (wmar/models/taming_wrapper.py:79-84): codes int64 [B, S*S]
 * -> images float [B, 3, R, R] (NCHW) clamped to [-1, 1]. */
int wmar_vq_decode(wmar_vq* v, const int64_t* codes_dev, int64_t B, float* images_dev, void* stream);
/* TamingARMMWrapper.images_to_codes (taming_wrapper.py:88-92): images float [B, 3, R, R] -> codes int64 [B, S*S].
 * prequant_dev (nullable): float [B*S*S, embed_dim], the vectors handed to the quantizer. */
int wmar_vq_encode(wmar_vq* v, const float* images_dev, int64_t B, int64_t* codes_dev, float* prequant_dev,
                   void* stream);

/* Probes (tests, debugging): one layer at a time through the loader and the dispatch the two calls above use, so that every kernel
 * variant can be compared with a float64 reference alone.  Activations cross them in the engine's own layout: NHWC fp32, channels
 * padded with zeros to a multiple of 8 (cin_s, cout_s).  Each probe allocates and frees its scratch and waits for the stream; none
 * of them is used by an engine path.  The text outputs name what the dispatch itself decided to launch.
 *
 * Convolution: w_dev [cout, cin, ks, ks] (torch layout, ks 1 or 3), bias_dev [cout] (nullable: zero), x_dev [B, Hs, Ws, cin_s],
 * res_dev (nullable) [B, Ho, Wo, cout_s] added in the epilogue, y_dev [B, Ho, Wo, cout_s].  Conventions as in the networks: pad 1 for
 * 3 x 3 stride 1, zero pad (0, 1, 0, 1) for stride 2, nearest x2 upsampling in front when up != 0.  gn_gamma_dev / gn_beta_dev [cin]
 * (nullable, together): GroupNorm(32, eps 1e-6) of x, followed by swish when gn_swish != 0, applied by the patch loader as in a
 * ResnetBlock (cin a multiple of 32, no upsampling).  out_mr_dev (nullable) float [B, 32, 2]: the (mean, rstd) the next GroupNorm on
 * y would be handed (cout a multiple of 32); arm_stats != 0 arms the per-tile statistics of the conv epilogue as decode / encode do,
 * and the text says which path delivered them.  kernel_buf: "conv=<kernel>;gn_in=<path>;stats=<path>". */
int wmar_vq_probe_conv(const float* w_dev, const float* bias_dev, int32_t cout, int32_t cin, int32_t ks, const float* x_dev,
                       const float* res_dev, const float* gn_gamma_dev, const float* gn_beta_dev, int32_t gn_swish, int64_t B, int32_t Hs,
                       int32_t Ws, int32_t stride, int32_t up, int32_t arm_stats, float* y_dev, float* out_mr_dev, char* kernel_buf,
                       int64_t buf_len, void* stream);
/* Attention core of an AttnBlock: q, k, v [B, H * W, C] -> o = softmax(q k^T C^-1/2) v.  path_buf: "path=bf16_pipe|scalar;scores=<kernel>;
 * pv=<kernel>". */
int wmar_vq_probe_attn(const float* q_dev, const float* k_dev, const float* v_dev, int64_t B, int32_t H, int32_t W, int32_t C, float* o_dev,
                       char* path_buf, int64_t buf_len, void* stream);
/* Nearest-code search: z_dev [P, E], codebook_dev [n_embed, E] -> codes_dev int64 [P], first minimum of |z|^2 + |e|^2 - 2 z.e.
 * path_buf: the search kernel and, for the split kernel, its number of code splits. */
int wmar_vq_probe_argmin(const float* z_dev, int64_t P, int32_t E, const float* codebook_dev, int32_t n_embed, int64_t* codes_dev,
                         char* path_buf, int64_t buf_len, void* stream);

/* Backward probes (wmar_amd/csrc/vq_grad.h): the backward of one layer alone, through the host functions a training engine would
 * call (make_dgrad_conv / run_conv_dgrad / run_conv_wgrad, run_gn_backward, attn_backward), in the layout of the probes above.  No
 * floating-point atomics anywhere: two calls on the same data give the same bits.
 *
 * Convolution (same four index maps as wmar_vq_probe_conv): w_dev [cout, cin, ks, ks], x_dev [B, Hs, Ws, cin_s] the conv's actual
 * input, gy_dev [B, Ho, Wo, cout_s] the gradient of its output -> gx_dev [B, Hs, Ws, cin_s] (padding channels 0), gw_dev
 * [cout, cin, ks, ks], gb_dev [cout].  The input gradient of a stride-1 conv is run_conv on the flipped, transposed weight (Hs, Ws --
 * 2 Hs, 2 Ws with up -- multiples of 8, as for any conv here), followed by a 2 x 2 sum with up; stride 2 has a gather kernel.  The
 * weight gradient is an fp32-input MFMA GEMM over K = B Ho Wo, split into K slices that a second launch adds in order.
 * gb_dev may be null (a bias-free conv, as the MaskGIT-VQGAN plan has them): the null goes to run_conv_wgrad, no bias kernel runs and
 * the call fails if the bias part of the workspace (allocated and filled with a sentinel either way) was written.
 * kernel_buf: "dgrad=<flip+conv kernel[+k_sum2x2] | k_dgrad_s2>;wgrad=<kernel>;splits=<K slices>;bgrad=<k_bgrad_partial | none>". */
int wmar_vq_probe_conv_backward(const float* w_dev, int32_t cout, int32_t cin, int32_t ks, const float* x_dev, const float* gy_dev, int64_t B,
                                int32_t Hs, int32_t Ws, int32_t stride, int32_t up, float* gx_dev, float* gw_dev, float* gb_dev,
                                char* kernel_buf, int64_t buf_len, void* stream);
/* GroupNorm(32, eps 1e-6), followed by swish when swish != 0: x_dev, gy_dev (gradient of the output), gx_dev [B, HW, C] (C a multiple
 * of 32), mr_dev float [B, 32, 2] the forward's (mean, rstd), gamma_dev / beta_dev [C] -> gx_dev, dgamma_dev [C], dbeta_dev [C].
 * path_buf: "path=<kernels>;chunks=<pixel chunks per image>". */
int wmar_vq_probe_gn_backward(const float* x_dev, const float* gy_dev, const float* mr_dev, const float* gamma_dev, const float* beta_dev,
                              int64_t B, int32_t HW, int32_t C, int32_t swish, float* gx_dev, float* dgamma_dev, float* dbeta_dev,
                              char* path_buf, int64_t buf_len, void* stream);
/* Attention core: runs the forward of wmar_vq_probe_attn (its softmax is the tape), then go_dev [B, H * W, C], the gradient of o ->
 * gq_dev, gk_dev, gv_dev [B, H * W, C].  path_buf: "path=bf16_pipe|plain;forward=bf16_pipe|scalar". */
int wmar_vq_probe_attn_backward(const float* q_dev, const float* k_dev, const float* v_dev, const float* go_dev, int64_t B, int32_t H, int32_t W,
                                int32_t C, float* gq_dev, float* gk_dev, float* gv_dev, char* path_buf, int64_t buf_len, void* stream);

/* Backward of the three layers only the MaskGIT-VQGAN plan has, each alone (no allocation, the stream is waited for, no engine path
 * calls them).  All three are exact in fp32: bit-equal to torch's fp32 autograd.
 * Average pool 2 x 2: gy_dev [B, Ho, Wo, C] (C a multiple of 4) -> gx_dev [B, 2 Ho, 2 Wo, C] = gy * 0.25 of the element's window. */
int wmar_vq_probe_avgpool_backward(const float* gy_dev, int64_t B, int32_t Ho, int32_t Wo, int32_t C, float* gx_dev, void* stream);
/* Decode edge, clamp(v, 0, 1) * 2 - 1: pre_dev [B, HW, Cs] the value v in front of the clamp (Cs >= C stored channels, a multiple of 4),
 * g_nchw_dev [B, C, HW] the image gradient -> g_nhwc_dev [B, HW, Cs] = 2 g where 0 <= v <= 1 (bounds included), 0 elsewhere and in the
 * padding channels. */
int wmar_mvq_probe_image_backward(const float* pre_dev, const float* g_nchw_dev, int64_t B, int32_t C, int32_t HW, int32_t Cs, float* g_nhwc_dev,
                                  void* stream);
/* Encode edge, (x + 1) / 2: g_nhwc_dev [B, HW, Cs] -> g_nchw_dev [B, C, HW] = g * 0.5. */
int wmar_mvq_probe_input_backward(const float* g_nhwc_dev, int64_t B, int32_t C, int32_t HW, int32_t Cs, float* g_nchw_dev, void* stream);

/* Trainable Taming VQGAN (wmar_amd/csrc/vq_train.h): encoder + quant_conv and post_quant_conv + decoder with a forward that records a
 * tape and a backward that delivers the input gradient and every conv / GroupNorm weight gradient (the codebook is frozen).  The
 * forwards make the launches of wmar_vq_encode / wmar_vq_decode in their order and are bit-equal to them (decode: before the clamp,
 * VQModel.decode).  Each half has a tape of its own -- one step can hold both -- sized at create time for cfg->max_batch images; no
 * call allocates.  Same checkpoint keys as wmar_vq_create (quantize.* is not read).
 *
 * set_weights repacks every weight in place (after an optimizer step) and invalidates both tapes.  A backward needs the tape of its
 * half: it returns WMAR_EINVAL (and leaves the engine usable) without a forward since create / set_weights or with a B other than the
 * forward's.  grad_images_dev / grad_zq_dev may be NULL when only weight gradients are wanted.  get_grads copies (accumulate == 0) or
 * adds (accumulate != 0) the torch-layout gradients of the named "<layer>.weight" / "<layer>.bias" tensors from the last backward of
 * their half.  Reductions have a fixed order everywhere: two runs give the same bits. */
typedef struct wmar_vq_train wmar_vq_train;
int wmar_vq_train_create(const wmar_vq_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream,
                         wmar_vq_train** out);
void wmar_vq_train_destroy(wmar_vq_train* t);
int64_t wmar_vq_train_device_bytes(const wmar_vq_train* t);
int wmar_vq_train_set_weights(wmar_vq_train* t, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream);
/* images_dev [B, 3, R, R] -> prequant_dev [B*S*S, embed_dim] = quant_conv(encoder(x)) */
int wmar_vq_train_encode(wmar_vq_train* t, const float* images_dev, int64_t B, float* prequant_dev, void* stream);
int wmar_vq_train_encode_backward(wmar_vq_train* t, const float* grad_prequant_dev, int64_t B, float* grad_images_dev, void* stream);
/* zq_dev [B*S*S, embed_dim] -> images_dev [B, 3, R, R], NOT clamped */
int wmar_vq_train_decode(wmar_vq_train* t, const float* zq_dev, int64_t B, float* images_dev, void* stream);
int wmar_vq_train_decode_backward(wmar_vq_train* t, const float* grad_images_dev, int64_t B, float* grad_zq_dev, void* stream);
int wmar_vq_train_get_grads(wmar_vq_train* t, const char* const* names, void* const* grads_dev, int32_t n, int32_t accumulate, void* stream);

/* --------------------------------------------------------------- MaskGIT-VQGAN (RAR's tokenizer)
 * deps/rar/modeling/modules/maskgit_vqgan.py + PretrainedTokenizer (deps/rar/modeling/titok.py:41-89).
 * Tensors by key name (encoder.*, decoder.*, quantize.embedding.weight).  Images cross this API in the
 * WRAPPER's convention, [-1, 1] (RarARMMWrapper.codes_to_images / images_to_codes, rar_wrapper.py:108-128). */
typedef struct wmar_mvq_config {
    int32_t hidden_channels, num_res_blocks, resolution, num_channels, z_channels, num_embeddings;
    int32_t n_levels;
    int32_t channel_mult[8];
    int32_t max_batch;
} wmar_mvq_config;

typedef struct wmar_mvq wmar_mvq;

int wmar_mvq_create(const wmar_mvq_config* cfg, const char* const* names, const void* const* tensors_dev,
                    int32_t n_tensors, void* stream, wmar_mvq** out);
void wmar_mvq_destroy(wmar_mvq* v);
int64_t wmar_mvq_device_bytes(const wmar_mvq* v);
int wmar_mvq_decode(wmar_mvq* v, const int64_t* codes_dev, int64_t B, float* images_dev, void* stream);
int wmar_mvq_encode(wmar_mvq* v, const float* images_dev, int64_t B, int64_t* codes_dev, float* prequant_dev,
                    void* stream);

/* Trainable MaskGIT-VQGAN (wmar_amd/csrc/vq_train.h): the plan of wmar_mvq_encode / wmar_mvq_decode as a wmar_vq_train handle, as RAR's
 * fine-tuning differentiates it (deps/rar/modeling/titok.py:91-208).  Every wmar_vq_train_* entry above serves the handle; the taped
 * forwards make the inference engine's launches in its order and are bit-equal to it.  For such a handle:
 *   - images cross in the wrapper's [-1, 1] convention, as for wmar_mvq_*;
 *   - wmar_vq_train_decode takes z_q rows [B*S*S, z_channels] and returns clamp(decoder(z_q), 0, 1) * 2 - 1; its backward passes the
 *     gradient where the taped value in front of the clamp lies in [0, 1] (bounds included) and multiplies it by 2;
 *   - wmar_vq_train_encode returns the encoder output rows [B*S*S, z_channels] of encoder((x + 1) / 2); its backward's image gradient
 *     carries the factor 0.5;
 *   - the convolutions inside the ResnetBlocks (conv1, conv2, nin_shortcut) and encoder.conv_in have no bias: set_weights needs none,
 *     and wmar_vq_train_get_grads on such a "<layer>.bias" returns WMAR_EINVAL naming the tensor and leaves the engine usable.
 * Same checkpoint keys as wmar_mvq_create (quantize.* is not read). */
int wmar_mvq_train_create(const wmar_mvq_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream,
                          wmar_vq_train** out);

/* Forward-only handles: the arguments of wmar_vq_train_create / wmar_mvq_train_create, a wmar_vq_train that serves
 * wmar_vq_train_encode, _decode, _set_weights, _device_bytes and _destroy.  The activations live in the plan's rotating and attention
 * slot buffers, as the inference engines' do; there is no per-tensor tape, no gradient slot, no weight-gradient buffer, no flipped or
 * dgrad weight pack, no backward scratch and no softmax tape.  The forward is the same executor on the same packed weights, so its
 * outputs are bit-equal to the taped handle's and to wmar_vq_* / wmar_mvq_*.  wmar_vq_train_encode_backward, _decode_backward and
 * _get_grads on such a handle return WMAR_EINVAL ("... a frozen handle ...") and leave it usable.  What a no-grad forward and the
 * original decoder of the fine-tuning loss run on. */
int wmar_vq_train_create_frozen(const wmar_vq_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors,
                                void* stream, wmar_vq_train** out);
int wmar_mvq_train_create_frozen(const wmar_mvq_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors,
                                 void* stream, wmar_vq_train** out);

/* ------------------------------------------------------------------------ LPIPS (wmar_amd/csrc/lpips.h)
 * The perceptual term of the tokenizer fine-tuning loss (deps/taming/modules/losses/lpips.py:41-122 in .eval()): a frozen VGG16
 * features[0:30] on two images, per-pixel normalised at five taps, the squared differences weighted by the lin layers, averaged over
 * the pixels and added in tap order.  The gradient goes to the first image (`input`) only; every weight is frozen.
 *
 * Tensors by the reference module's key names: scaling_layer.shift / .scale [1, 3, 1, 1]; net.slice1.0 / .2, net.slice2.5 / .7,
 * net.slice3.10 / .12 / .14, net.slice4.17 / .19 / .21, net.slice5.24 / .26 / .28 each with .weight [cout, cin, 3, 3] and .bias;
 * lin0 .. lin4 as lin<k>.model.1.weight [1, chns[k], 1, 1].  chns: the five slice widths (multiples of 8; VGG16 has 64, 128, 256,
 * 512, 512).  resolution: a multiple of 128 (relu5_3 is resolution / 16 and the convolutions work on 8 x 8 tiles).
 *
 * All memory is allocated at create time for max_batch image pairs; no call allocates.  Reductions have a fixed order everywhere and
 * there are no floating-point atomics: two runs give the same bits.  Images are [B, 3, S, S] fp32, contiguous. */
typedef struct wmar_lpips_config {
    int32_t chns[5];
    int32_t resolution;
    int32_t max_batch;
} wmar_lpips_config;

typedef struct wmar_lpips wmar_lpips;
int wmar_lpips_create(const wmar_lpips_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream,
                      wmar_lpips** out);
void wmar_lpips_destroy(wmar_lpips* h);
int64_t wmar_lpips_device_bytes(const wmar_lpips* h);
/* value_dev [B] = LPIPS(input, target) per image; per_tap_dev [5, B] (may be NULL) the five terms it is the sum of.  keep_tape != 0
 * keeps what the backward needs (the post-ReLU activations of the input branch, the normalised taps of the target branch); every
 * forward replaces the tape of the one before. */
int wmar_lpips_forward(wmar_lpips* h, const float* input_dev, const float* target_dev, int64_t B, int32_t keep_tape, float* value_dev,
                       float* per_tap_dev, void* stream);
/* grad_input_dev [B, 3, S, S] = sum_b grad_value_dev[b] d value[b] / d input.  WMAR_EINVAL (engine still usable) when the last
 * forward kept no tape or ran another B. */
int wmar_lpips_backward(wmar_lpips* h, const float* grad_value_dev, int64_t B, float* grad_input_dev, void* stream);

/* One new layer alone, through the host functions the engine calls (the stream is waited for).  Activations NHWC fp32.
 * Input edge: x_dev [B, 3, HW] -> y_dev [B, HW, 8] = (x - shift) / scale (fp32 subtract, fp32 divide; padding channels 0); its backward
 * g_nhwc_dev [B, HW, 8] -> g_nchw_dev [B, 3, HW] = g / scale.  Both bit-equal to torch's fp32 result. */
int wmar_lpips_probe_input(const float* x_dev, const float* shift_dev, const float* scale_dev, int64_t B, int32_t HW, float* y_dev, void* stream);
int wmar_lpips_probe_input_backward(const float* g_nhwc_dev, const float* scale_dev, int64_t B, int32_t HW, float* g_nchw_dev, void* stream);
/* ReLU + 2 x 2 stride-2 max-pool: x_dev [B, H, W, C] (C a multiple of 4, H and W even) -> y_dev = relu(x) (may be x_dev) and p_dev
 * [B, H / 2, W / 2, C]; p_dev NULL runs the ReLU alone.  relu(x) = x < 0 ? 0 : x: -0.0 and NaN pass, as through torch's relu.
 * Backward at the taped y_dev: gp_dev (gradient of p) goes to the first maximum of its window in row-major order, gt_dev (gradient
 * reaching y directly; may be NULL) is added, the sum passes where y > 0 -> gx_dev (may be gt_dev).  gp_dev NULL: the ReLU alone on
 * gt_dev.  Bit-equal to torch's fp32 autograd. */
int wmar_lpips_probe_relu_pool(const float* x_dev, int64_t B, int32_t H, int32_t W, int32_t C, float* y_dev, float* p_dev, void* stream);
int wmar_lpips_probe_relu_pool_backward(const float* y_dev, const float* gp_dev, const float* gt_dev, int64_t B, int32_t H, int32_t W, int32_t C,
                                        float* gx_dev, void* stream);
/* The head of one tap: f0_dev, f1_dev [B, HW, C] (C a multiple of 4, at most 1024), w_dev [C] -> value_dev [B], the mean over pixels
 * of sum_c w_c (n0_c - n1_c)^2 with n = f / (sqrt(sum_c f^2) + 1e-10); its backward grad_value_dev [B] -> g0_dev [B, HW, C], the
 * gradient towards f0 only, exactly 0 at a pixel whose f0 is all zero. */
int wmar_lpips_probe_head(const float* f0_dev, const float* f1_dev, const float* w_dev, int64_t B, int32_t HW, int32_t C, float* value_dev,
                          void* stream);
int wmar_lpips_probe_head_backward(const float* f0_dev, const float* f1_dev, const float* w_dev, const float* grad_value_dev, int64_t B, int32_t HW,
                                   int32_t C, float* g0_dev, void* stream);

/* ------------------------------------------------------------------------ evaluation transforms (harness)
 * wmar/augmentations/valuemetric.py:41-140, geometric.py:22-117 as applied by generate.py:142-164: one launch over the whole batch
 * [B, C, H, W] (fp32, contiguous).  op: 0 identity, 1 Gaussian blur (p0 = odd kernel size), 2 Gaussian noise (p0 = standard deviation,
 * noise_dev = standard normal draws of the image shape), 3 brightness (p0 = factor), 4 rotation (p0 = counter-clockwise quarter turns,
 * p1 = remainder in degrees, [0, 90)), 5 horizontal flip, 6 upper-left crop of p0 x p1 pixels resized back (antialiased bilinear),
 * 7 the same crop padded back with zeros.  pm1 != 0: pixels cross this call in [-1, 1] (the decoder's range) and are transformed in
 * [0, 1] and clamped, as generate.py:146-150 does around every transform.  JPEG is wmar_jpeg below. */
int wmar_augment(int32_t op, const float* in_dev, float* out_dev, const float* noise_dev, int64_t B, int32_t C, int32_t H,
                 int32_t W, int32_t pm1, double p0, double p1, void* stream);

/* The vector-Jacobian product of wmar_augment as it is implemented, range change and clamp included (training through the transforms,
 * finetune.py): grad_in = J^T grad_out at the forward input `in_dev`.  op, noise_dev, pm1, p0 and p1 mean what they mean to
 * wmar_augment; all buffers are [B, C, H, W] fp32, contiguous.  The clamp passes the gradient where 0 <= t <= 1, both bounds included
 * (as torch.clamp), with t recomputed by the forward's own arithmetic; the noise draws get no gradient.  Gather form, no atomics: two
 * calls return the same bits.  `workspace_dev`: B * C * H * W floats, required for blur (two launches), NULL otherwise.  grad_in_dev
 * may be grad_out_dev only for identity, noise, brightness and crop + pad.  Every argument is checked before the first launch. */
int wmar_augment_backward(int32_t op, const float* in_dev, const float* grad_out_dev, float* grad_in_dev, const float* noise_dev,
                          float* workspace_dev, int64_t B, int32_t C, int32_t H, int32_t W, int32_t pm1, double p0, double p1,
                          void* stream);

/* JPEG round trip at `quality` (1..100), valuemetric.py:30-75: bit for bit the pixels PIL's save(format="JPEG", quality=q) +
 * Image.open(...).convert("RGB") return (libjpeg-turbo's baseline path: 4:2:0, integer DCT, fancy upsampling), computed without a
 * bitstream.  [B, 3, H, W] fp32 in [0, 1] (clamped on entry), H and W multiples of 16; buffers 16-byte aligned, in != out.
 * passthrough != 0: the output is x + (jpeg(x) - x) in fp32, as the module's straight-through form, else jpeg(x); clamped to [0, 1].
 * pm1 != 0: pixels cross the call in [-1, 1], as wmar_augment.  Two launches; `workspace_dev` holds the reconstructed Y / Cb / Cr
 * samples in between: at least wmar_jpeg_workspace_bytes(B, H, W) bytes (0 if the kernel needs none), owned by the caller. */
int64_t wmar_jpeg_workspace_bytes(int64_t B, int32_t H, int32_t W);
int wmar_jpeg(const float* in_dev, float* out_dev, void* workspace_dev, int64_t workspace_bytes, int64_t B, int32_t H, int32_t W,
              int32_t quality, int32_t pm1, int32_t passthrough, void* stream);

/* ------------------------------------------------------------------------ image ingest
 * ImageTokenizer.img_tokens_from_pil up to the VQGAN (deps/chameleon/inference/image_tokenizer.py:51-98): _whiten_transparency, then
 * _vqgan_input_from = PIL's resize(LANCZOS) to short side `target`, centre crop, u8 / 255 * 2 - 1 -- for a batch of 8-bit images of
 * any sizes, bit for bit what PIL returns (Pillow's 8-bit resample is integer arithmetic on coefficient tables built in double).
 *
 * wmar_resample_coeffs (host only): Pillow's LANCZOS tables for one axis of in_size -> out_size pixels and the output window
 * [out0, out0 + n_out): first input pixel xmin_out and tap count count_out, int32 [n_out] each; 22-bit fixed-point weights k_out int32
 * [n_out * ksize] (row i = the taps of output out0 + i, zero beyond its count); *ksize_out = ceil(support) * 2 + 1.  k_capacity:
 * entries k_out holds; in_size up to 32768. */
int wmar_resample_coeffs(int32_t in_size, int32_t out_size, int32_t out0, int32_t n_out, int32_t* xmin_out, int32_t* count_out,
                         int32_t* k_out, int32_t k_capacity, int32_t* ksize_out);

/* One image of a batch: `offset` bytes into the pixel buffer, width x height pixels of `channels` bytes, row-major (HWC).  The resized
 * size and the crop origin are the caller's: the reference computes them with Python's round() (half to even) and //. */
typedef struct wmar_image_desc {
    int64_t offset;
    int32_t width, height, channels; /* 3 = RGB, 4 = RGBA (blended over white first) */
    int32_t new_width, new_height, crop_x0, crop_y0;
} wmar_image_desc;

/* pixels_dev: uint8 images back to back, 4-byte aligned, pixels_bytes in total; desc_host: n descriptors on the host, every one
 * validated against pixels_bytes and its own resized size (sides 1..32768, channels 3 | 4, crop window of target x target inside the
 * resized image) BEFORE anything is launched: WMAR_EINVAL names the image.  out_dev float [n, 3, target, target] in [-1, 1];
 * out_u8_dev (nullable) uint8 [n, target, target, 3], the cropped 8-bit image.  Only the crop window is computed.  Two launches per
 * batch.  The tables and the 8-bit intermediate between the passes live in a per-device scratch buffer the library keeps and grows
 * (the whitening table is uploaded when it is allocated); the call waits for its launches, and calls on one device take turns. */
int wmar_image_ingest(const uint8_t* pixels_dev, int64_t pixels_bytes, const wmar_image_desc* desc_host, int64_t n, int32_t target,
                      float* out_dev, uint8_t* out_u8_dev, void* stream);

/* The two entries above with the resampling filter as an argument (Pillow's numbers, Image.Resampling).  BILINEAR is Pillow's triangle
 * filter 1 - |x| on |x| < 1 with support 1 (src/libImaging/Resample.c, bilinear_filter): what torchvision's Resize(interpolation =
 * BILINEAR) applies to a PIL image, as the reference's precompute_imagenet_codes.py does.  Everything else -- the stretch by
 * max(in / out, 1), the normalisation, the 22-bit rounding, the two integer passes, the unfiltered unchanged axis -- is shared, so
 * wmar_resample_coeffs(...) == wmar_resample_coeffs_filtered(..., WMAR_RESAMPLE_LANCZOS) and likewise for the ingest.  Any other
 * filter value is WMAR_EINVAL before anything is computed. */
#define WMAR_RESAMPLE_LANCZOS 1
#define WMAR_RESAMPLE_BILINEAR 2
int wmar_resample_coeffs_filtered(int32_t in_size, int32_t out_size, int32_t out0, int32_t n_out, int32_t* xmin_out, int32_t* count_out,
                                  int32_t* k_out, int32_t k_capacity, int32_t* ksize_out, int32_t filter);
int wmar_image_ingest_filtered(const uint8_t* pixels_dev, int64_t pixels_bytes, const wmar_image_desc* desc_host, int64_t n, int32_t target,
                               float* out_dev, uint8_t* out_u8_dev, int32_t filter, void* stream);

/* ------------------------------------------------------------------------ synchronisation layer (WAM geometry fit)
 * wmar/watermarking/synchronization.py: the device half of WamSync.remove_sync.  All tensors contiguous; images and label maps are
 * square, S x S.  No call waits for its launches; workspaces are the caller's.
 *
 * wmar_sync_positions: estimate_augmentation_with_wam :224-243 for a batch.  preds_dev fp32 [B, 33, S, S] (channel 0 the mask logit,
 * 1..32 the bit logits, already at the image size); positions_dev int8 [B, S, S] in {-1, 0, 1, 2, 3}: the nearest of the four fixed
 * messages 0^32, 0^16 1^16, 1^16 0^16, 1^32 by Hamming distance of `logit > 0` (first minimum), kept when the distance is <= 6 and
 * fp32 sigmoid(mask logit) > 0.5 as torch evaluates it (false at 5e-8, true at 2e-7), else -1; sizes_dev int32 [B, 4] pixels per
 * message (zeroed by the call).  One launch. */
int wmar_sync_positions(const float* preds_dev, int64_t B, int32_t S, int8_t* positions_dev, int32_t* sizes_dev, void* stream);

/* wmar_sync_fit: fit_best_aug + rotate_wm + find_cut (:90-201) for a batch of label maps positions_dev int8 [B, S, S] (0..3; anything
 * else is background), 4 <= S <= 512.  aug_dev int32 [B, 4] = (rotation in degrees, cut_i, cut_j, flipped); total_error_dev
 * (nullable) fp64 [B, 41] = errori + errorj of the angles -20..20 (1e9 per axis without signal).  Exactness contract: every pixel of
 * the 41 x 4 rotated masks is thresholded on the fp64 value scipy.ndimage.rotate(order=3, mode="constant", reshape=False)
 * interpolates (cubic B-spline prefilter with mirror initialisation, 4 x 4 taps), summed in scipy's order without contraction; a
 * value closer than ~1e-12 to 0.5 may fall on either side.  Counts, thresholds (40 at S = 256, else 80), cumulative sums, the
 * cut / flip search, its half-to-even roundings and the selection across angles are integer / fp64 restatements without tolerance.
 * workspace_dev (16-byte aligned): error and cut tables of the batch plus the spline coefficients fp64 [n, S, S, 4] of as many
 * images n as fit; wmar_sync_workspace_bytes(B, S) holds the whole batch (four launches), a smaller one (at least the tables plus
 * one image) makes the call walk the batch in chunks of three launches each.  B <= 65535.
 * Result region (part of the contract; tests read it): once the call's launches have finished, the workspace starts with
 *   err  fp64  [B, 41]      errori + errorj of every angle -20..20 (what total_error_dev receives), then, without padding,
 *   cut  int32 [B, 41, 3]   (cut_i, cut_j, flipped_j) find_cut returned at that angle: S / 2 and 0 where an axis has no weight;
 * B * 41 * 20 bytes, rounded up to a multiple of 256, in front of the coefficients.  aug_dev is selected from these tables. */
int64_t wmar_sync_workspace_bytes(int64_t B, int32_t S);
int wmar_sync_fit(const int8_t* positions_dev, int64_t B, int32_t S, int32_t* aug_dev, double* total_error_dev, void* workspace_dev,
                  int64_t workspace_bytes, void* stream);

/* wmar_sync_rotate_labels (tests, debugging): rotate_wm of one angle (whole degrees): out_dev uint8 [B, S, S], the thresholded masks
 * of labels 1..4 merged in ascending order (0 = background).  Workspace as wmar_sync_fit. */
int wmar_sync_rotate_labels(const int8_t* positions_dev, int64_t B, int32_t S, int32_t angle, uint8_t* out_dev, void* workspace_dev,
                            int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------ synchronisation layer (WAM embedder)
 * deps/watermark_anything: models/embedder.py VAEEmbedder (modules/vae.py VAEEncoder / VAEDecoder with tanh_out, modules/
 * msg_processor.py "binary+concat"), modules/jnd.py JND (in_channels 1, out_channels 3) and models/wam.py Wam.blend / Wam.embed, for
 * images of the network's own size (no resize).  Tensors by key name relative to `embedder.` (encoder.*, decoder.*,
 * msg_processor.msg_embeddings.weight [2 nbits, 2 nbits]).  The network runs through the VQGAN engines' layer plan and kernels
 * (csrc/vq_plan.h plan_wam); refused with a text: ch % 32 != 0, a latent size that is not a multiple of 8, nbits outside 1..64.
 * max_batch counts decoder rows (one per image and message); longer calls are walked in chunks.  attenuation: 0 none, 1 jnd_1_3,
 * 2 jnd_1_3_blue, applied in [0, 1] space between unnormalize_img and normalize_img (utils/inference_utils.py:64).  Images are
 * float [B, 3, R, R] (NCHW), messages int32 (a bit is set when it is not 0).  R other than `resolution` is WMAR_EINVAL and nothing
 * is launched.  No call but the probes waits for its launches; two runs give the same bits. */
typedef struct wmar_wam_config {
    int32_t ch, num_res_blocks, resolution, z_channels, nbits;
    int32_t n_levels;
    int32_t ch_mult[8];
    int32_t n_attn_res;
    int32_t attn_resolutions[8];
    int32_t max_batch;
    float scaling_w, scaling_i;
    int32_t attenuation;
} wmar_wam_config;

typedef struct wmar_wam wmar_wam;

int wmar_wam_create(const wmar_wam_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream,
                    wmar_wam** out);
void wmar_wam_destroy(wmar_wam* w);
int64_t wmar_wam_device_bytes(const wmar_wam* w);

/* Wam.embed (models/wam.py:147-192): imgs_norm_dev in WAM-normalised space, msgs_dev int32 [B, nbits] (one message per image) ->
 * imgs_w_dev [B, 3, R, R] = blend(imgs, preds_w), preds_w_dev (nullable) [B, 3, R, R] = tanh(decoder output).  No clamp. */
int wmar_wam_embed(wmar_wam* w, const float* imgs_norm_dev, int64_t B, int32_t R, const int32_t* msgs_dev, float* imgs_w_dev,
                   float* preds_w_dev, void* stream);
/* WamSync.add_sync (wmar/watermarking/synchronization.py:299-316): imgs_pm1_dev in [-1, 1], msgs_dev int32 [K, nbits], masks_dev uint8
 * [K, R, R] of 0 / 1 (the caller checks), 1 <= K <= 8.  Normalise, one encoder pass per image, one decoder row per (image, message),
 * blend in message order -- a later mask overrides an earlier one, as multi * (1 - m) + w * m does for 0 / 1 masks; where no mask is
 * set the image itself -- then unnormalise, * 2 - 1, clamp to [-1, 1] into out_pm1_dev [B, 3, R, R]. */
int wmar_wam_add_sync(wmar_wam* w, const float* imgs_pm1_dev, int64_t B, int32_t R, const int32_t* msgs_dev, int32_t K,
                      const uint8_t* masks_dev, float* out_pm1_dev, void* stream);

/* Probes (tests, debugging): one kernel of the embedder at a time; none is used by an engine path; each waits for the stream.
 * wmar_wam_probe_jnd: imgs01_dev [B, 3, R, R] in [0, 1], R a multiple of 4 -> heat_dev [B, R, R] = JND.heatmaps / its one channel
 * (the blue weights (0.5, 0.5, 1.0) belong to the tail).
 * wmar_wam_probe_latent_msg: the decoder input out_dev [rows, S, S, pad8(z_channels + 2 nbits)] (NHWC): row r takes its first
 * z_channels channels from image r / img_div of latents_dev [n_images, S, S, pad8(z_channels)], the next 2 nbits channels from
 * sum_j table[2 j + bit_j] (ascending j, fp32) of message (msg_mod ? r % msg_mod : r) of msgs_dev int32 [n_msgs, nbits]; padding 0.
 * wmar_wam_probe_tail: the tail on given decoder outputs y_dev [rows, R, R, 8] (NHWC, 3 real channels) and images imgs_dev
 * [B, 3, R, R] (in_mode 1: WAM-normalised, 2: in [-1, 1]).  masks_dev null: embed form, rows = B, out_dev [B, 3, R, R] = imgs_w and
 * preds_dev (nullable) = tanh(y).  masks_dev uint8 [K, R, R]: add_sync form, rows = B * K (row = image * K + message), out_dev in
 * [-1, 1].  The heat maps (attenuation != 0) are computed by the call. */
int wmar_wam_probe_jnd(const float* imgs01_dev, int64_t B, int32_t R, float* heat_dev, void* stream);
int wmar_wam_probe_latent_msg(const float* latents_dev, int64_t n_images, int32_t S, int32_t z_channels, int32_t nbits,
                              const float* table_dev, const int32_t* msgs_dev, int64_t n_msgs, int64_t rows, int32_t img_div,
                              int32_t msg_mod, float* out_dev, void* stream);
int wmar_wam_probe_tail(const float* y_dev, const float* imgs_dev, int32_t in_mode, int64_t B, int32_t R, const uint8_t* masks_dev,
                        int32_t K, float scaling_w, float scaling_i, int32_t attenuation, float* out_dev, float* preds_dev, void* stream);

/* ------------------------------------------------------------------------ synchronisation layer (WAM extractor)
 * deps/watermark_anything: models/extractor.py SegmentationExtractor = modules/vit.py ImageEncoderViT (sam_base of configs/
 * extractor.yaml: patch embedding + pos_embed, blocks of windowed / global attention with decomposed relative positions, mlp_ratio 4,
 * the neck) + modules/pixel_decoder.py PixelDecoder (bilinear Upsample stages, last_layer) -- models/wam.py Wam.detect for images of
 * the network's own size (no resize).  Tensors by key name relative to `detector.` (image_encoder.*, pixel_decoder.*).
 * global_attn_indexes: the blocks that attend over the whole grid; the others inside window_size x window_size windows.
 * wmar_wamx_create refuses, with a text: a grid (img_size / patch_size) that is no multiple of window_size (the reference pads such
 * grids with zero tokens that take part as keys; not built); a grid that is no multiple of the 8 x 8 conv tile, a patch size that is
 * no multiple of 4; embed_dim % num_heads != 0, a head width that is no multiple of 4 or above 64, windows above 32 x 32 or K and V of
 * a window beyond the LDS; upscaling factors other than 2, 4, 8, a product other than patch_size, out_chans not divisible by it; nbits
 * outside 1..64; a missing tensor (WMAR_EMISSING, the text names it).  The ABI carries no tensor shapes: that each rel_pos table has
 * 2 S - 1 rows (S the block's window or grid size; get_rel_pos then never interpolates) is checked by the caller (wam_extractor.py).
 * Images float [B, 3, R, R] in WAM-normalised space -> preds float [B, nbits + 1, R, R] (NCHW; channel 0 the mask logit, then the
 * bit logits; no sigmoid).  The batch is walked in groups of max_batch; no value crosses a group, so the chunking changes no bit.
 * R other than img_size is WMAR_EINVAL, nothing is launched and the output is untouched.  No call but the probes waits for its
 * launches; two runs give the same bits. */
typedef struct wmar_wamx_config {
    int32_t img_size, patch_size, embed_dim, depth, num_heads, window_size;
    int32_t n_global;
    int32_t global_attn_indexes[16];
    int32_t out_chans;
    int32_t n_stages;
    int32_t upscale_stages[4];
    int32_t nbits;
    int32_t max_batch;
} wmar_wamx_config;

typedef struct wmar_wamx wmar_wamx;

int wmar_wamx_create(const wmar_wamx_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream,
                     wmar_wamx** out);
void wmar_wamx_destroy(wmar_wamx* w);
int64_t wmar_wamx_device_bytes(const wmar_wamx* w);
int wmar_wamx_detect(wmar_wamx* w, const float* imgs_norm_dev, int64_t B, int32_t R, float* preds_dev, void* stream);

/* Probes (tests, debugging): one kernel of the extractor at a time, through the launches the engine uses; each waits for the stream.
 * Activations are NHWC with channels padded to a multiple of 8 (padding zero), written pad8(C) below.
 * wmar_wamx_probe_layernorm: x_dev [n, pad8(C)] -> mr_dev float [n, 2] = (mean, 1 / sqrt(biased variance + eps)) per token over its C
 * channels (the normalisation itself is applied by the consuming conv while it stages its patch).
 * wmar_wamx_probe_patch_embed: imgs_dev [B, 3, R, R], w_dev [D, 3, patch, patch], bias_dev [D], pos_dev [R / patch, R / patch, D]
 * -> out_dev [B, R / patch, R / patch, D] = conv + bias + pos.
 * wmar_wamx_probe_attn: qkv_dev [B, grid, grid, 3 * num_heads * head_dim] (channel which * D + head * head_dim + c), windows of
 * S x S tokens (S = grid: global), rel_h_dev / rel_w_dev [2 S - 1, head_dim] -> out_dev [B, grid, grid, num_heads * head_dim].
 * wmar_wamx_probe_upstage: x_dev [B, Hs, Hs, pad8(Cin)], optionally LayerNorm(eps 1e-6; gamma / beta [Cin]) (+ GELU if ln_gelu) of
 * it, bilinear upsampling by f, ReflectionPad2d(1), 3 x 3 conv w_dev [Cout, Cin, 3, 3] without bias -> out_dev
 * [B, Hs f, Hs f, pad8(Cout)] (the stage's own LayerNorm + GELU are applied by the NEXT conv).
 * wmar_wamx_probe_last: x_dev [B, H, H, pad8(Cin)], the same optional LayerNorm (+ GELU), 1 x 1 conv w_dev [Cout, Cin, 1, 1] +
 * bias_dev -> out_dev [B, Cout, H, H] (NCHW).
 * wmar_wamx_probe_block: block `block` of an engine (norm1 .. MLP residual) on x_dev [B, grid, grid, embed_dim], B <= max_batch ->
 * out_dev of the same shape. */
int wmar_wamx_probe_layernorm(const float* x_dev, int64_t n, int32_t C, float eps, float* mr_dev, void* stream);
int wmar_wamx_probe_patch_embed(const float* imgs_dev, int64_t B, int32_t R, int32_t patch, const float* w_dev, const float* bias_dev,
                                const float* pos_dev, int32_t D, float* out_dev, void* stream);
int wmar_wamx_probe_attn(const float* qkv_dev, int64_t B, int32_t grid, int32_t S, int32_t num_heads, int32_t head_dim, const float* rel_h_dev,
                         const float* rel_w_dev, float* out_dev, void* stream);
int wmar_wamx_probe_upstage(const float* x_dev, int64_t B, int32_t Hs, int32_t Cin, int32_t f, const float* ln_gamma_dev,
                            const float* ln_beta_dev, int32_t ln_gelu, const float* w_dev, int32_t Cout, float* out_dev, void* stream);
int wmar_wamx_probe_last(const float* x_dev, int64_t B, int32_t H, int32_t Cin, const float* ln_gamma_dev, const float* ln_beta_dev,
                         int32_t ln_gelu, const float* w_dev, const float* bias_dev, int32_t Cout, float* out_dev, void* stream);
int wmar_wamx_probe_block(wmar_wamx* w, int32_t block, const float* x_dev, int64_t B, float* out_dev, void* stream);

/* ------------------------------------------------------------------------ exchange step (RCCL over xGMI)
 * The sharded job (one process per GPU; rank r == the reference's `--chunk_id r --num_chunks world`, generate.py:204, :304) has no
 * data-path collective.  Its two exchanges -- the finished key table from rank 0 once, the per-image records once per step
 *  -- as thin RCCL wrappers; RCCL is resolved at run time so that a process that already carries one
 * (PyTorch-ROCm) keeps exactly that copy.  `id` is RCCL's 128-byte unique id: made on one rank, handed to the others by the host
 * (file, store, environment).  Buffers are device pointers, sizes in bytes; the calls are asynchronous on `stream`. */
typedef struct wmar_comm wmar_comm;
#define WMAR_COMM_ID_BYTES 128
int wmar_comm_unique_id(void* id_out, int64_t id_bytes);
int wmar_comm_init(const void* id, int64_t id_bytes, int32_t rank, int32_t world, wmar_comm** out);
int wmar_comm_bcast(wmar_comm* c, void* buf_dev, int64_t bytes, int32_t root, void* stream);
/* recv_dev holds world x bytes_per_rank, rank order */
int wmar_comm_allgather(wmar_comm* c, const void* send_dev, void* recv_dev, int64_t bytes_per_rank, void* stream);
int32_t wmar_comm_rank(const wmar_comm* c);
int32_t wmar_comm_world(const wmar_comm* c);
void wmar_comm_destroy(wmar_comm* c);

#ifdef __cplusplus
}
#endif
#endif /* WMAR_HIP_H */
