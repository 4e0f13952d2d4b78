// Gumbel-key ("Aaronson") sampler and detector score -- SURVEY.md section 8a row G1.
//
// Reference: wmar_audio/watermark/engine.py:29-75 (gumbel_sample) and :123-134
// (gumbel_score_tok).  The reference's image code never calls them: RAR + Gumbel key is an
// extension whose semantics follow that file with a fixed key (ngram = 0, engine.py:17-18).
//
// One workgroup per row, the row in registers (V <= 16384).  Every sum is the order-independent
// fixed-point sum of include/wmar_math.h and the two order statistics (top-p cut, k-th largest)
// are bisections over a composite key (probability bits, then lower index first), so a row's
// result does not depend on how it is laid over the lanes (the CPU checker restates the same
// arithmetic and must agree bit for bit).  Compile with -ffp-contract=off.
#include "sampler.h"
#include "../../include/wmar_math.h"

namespace wmar {

constexpr int GUM_THREADS = 1024;
constexpr int GUM_WAVES = GUM_THREADS / 64;
constexpr int GUM_EPT = 16;
constexpr int GUM_IDX_BITS = 14;
constexpr float GUM_UNDERFLOW = -103.972077f;   // log(2^-150): below this fp32 pow(rs, 1/p) is exactly 0

__device__ __forceinline__ unsigned long long gum_block_sum(unsigned long long v, unsigned long long* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long s = 0;
    for (int i = 0; i < GUM_WAVES; ++i) s += red[i];
    return s;
}

__device__ __forceinline__ unsigned long long gum_ckey(float p, int v) {
    return ((unsigned long long)wmar_f32_key(p) << GUM_IDX_BITS) | (unsigned long long)((1 << GUM_IDX_BITS) - 1 - v);
}

__global__ __launch_bounds__(GUM_THREADS) void k_gumbel_sample(GumbelArgs a) {
    __shared__ unsigned long long red[GUM_WAVES];
    __shared__ float red_f[GUM_WAVES];
    __shared__ unsigned long long red_k[GUM_WAVES];
    const long long b = blockIdx.x;
    const int V = (int)a.V;
    const int tid = threadIdx.x;
    const long long step = a.step_dev ? (long long)*a.step_dev : 0;
    const long long t = a.t_dev ? (long long)*a.t_dev : 0;
    const float* lg = a.logits + b * a.V;
    const float* ul = a.logits_uncond ? a.logits_uncond + b * a.V : nullptr;
    const float cfg = ul ? a.cfg_scale[step] : 0.f;
    const float* lr = a.log_rs + b * a.key_row_stride;

    float x[GUM_EPT];
    const bool sampling = a.use_sampling && a.temp > 0.0f;
#pragma unroll
    for (int i = 0; i < GUM_EPT; ++i) {
        const int v = tid + i * GUM_THREADS;
        float xv = -INFINITY;
        if (v < V) {
            xv = lg[v];
            if (ul) { const float u = ul[v]; const float dlt = xv - u; const float sc = dlt * cfg; xv = u + sc; }
            if (sampling) xv = xv / a.temp;
        }
        x[i] = xv;
    }
    // row maximum (and, without sampling, its first index: torch.argmax)
    unsigned long long best = 0;
#pragma unroll
    for (int i = 0; i < GUM_EPT; ++i) {
        const int v = tid + i * GUM_THREADS;
        if (v < V) best = max(best, gum_ckey(x[i], v));
    }
    for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned long long)__shfl_xor((long long)best, o));
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    best = 0;
    for (int i = 0; i < GUM_WAVES; ++i) best = max(best, red[i]);
    __syncthreads();
    long long token;
    if (!sampling) {
        token = (1 << GUM_IDX_BITS) - 1 - (long long)(best & ((1u << GUM_IDX_BITS) - 1));
    } else {
        const float m = wmar_key_f32((uint32_t)(best >> GUM_IDX_BITS));
        float p[GUM_EPT];
        unsigned long long z = 0;
#pragma unroll
        for (int i = 0; i < GUM_EPT; ++i) {
            const int v = tid + i * GUM_THREADS;
            p[i] = v < V ? wmar_expf(x[i] - m) : 0.f;
            z += wmar_fx(p[i]);
        }
        const float Z = wmar_fx_to_f32(gum_block_sum(z, red));
#pragma unroll
        for (int i = 0; i < GUM_EPT; ++i) p[i] = p[i] / Z;

        const bool by_rank = a.top_p > 0.0f;      // ties of the race resolve in sorted order (engine.py:69-74)
        if (a.top_p > 0.0f) {
            // smallest composite key K with mass{ckey > K} <= top_p: everything from K upwards is kept
            unsigned long long lo = 0, hi = (1ull << (32 + GUM_IDX_BITS)) - 1;
            while (lo < hi) {
                const unsigned long long mid = lo + ((hi - lo) >> 1);
                unsigned long long ms = 0;
#pragma unroll
                for (int i = 0; i < GUM_EPT; ++i) {
                    const int v = tid + i * GUM_THREADS;
                    if (v < V && gum_ckey(p[i], v) > mid) ms += wmar_fx(p[i]);
                }
                ms = gum_block_sum(ms, red);
                if (wmar_fx_to_f32(ms) > a.top_p) lo = mid + 1; else hi = mid;
            }
            unsigned long long ks = 0;
#pragma unroll
            for (int i = 0; i < GUM_EPT; ++i) {
                const int v = tid + i * GUM_THREADS;
                if (!(v < V && gum_ckey(p[i], v) >= lo)) p[i] = 0.f;
                ks += wmar_fx(p[i]);
            }
            const float S = wmar_fx_to_f32(gum_block_sum(ks, red));
#pragma unroll
            for (int i = 0; i < GUM_EPT; ++i) p[i] = p[i] / S;
        } else if (a.top_k > 0) {
            const unsigned long long kk = (unsigned long long)min((long long)a.top_k, (long long)V);
            // largest composite key K with count{ckey >= K} >= k
            unsigned long long lo = 0, hi = (1ull << (32 + GUM_IDX_BITS)) - 1;
            while (lo < hi) {
                const unsigned long long mid = lo + ((hi - lo + 1) >> 1);
                unsigned long long c = 0;
#pragma unroll
                for (int i = 0; i < GUM_EPT; ++i) {
                    const int v = tid + i * GUM_THREADS;
                    if (v < V && gum_ckey(p[i], v) >= mid) ++c;
                }
                c = gum_block_sum(c, red);
                if (c >= kk) lo = mid; else hi = mid - 1;
            }
            unsigned long long ks = 0;
#pragma unroll
            for (int i = 0; i < GUM_EPT; ++i) {
                const int v = tid + i * GUM_THREADS;
                if (v < V) {
                    if (!(gum_ckey(p[i], v) >= lo)) p[i] = 1e-6f;
                    ks += wmar_fx(p[i]);
                }
            }
            const float S = wmar_fx_to_f32(gum_block_sum(ks, red));
#pragma unroll
            for (int i = 0; i < GUM_EPT; ++i) p[i] = p[i] / S;
        }
        // the race
        float bs = -INFINITY;
        unsigned long long bk = 0;      // tie order: larger is earlier
        bool have = false;
#pragma unroll
        for (int i = 0; i < GUM_EPT; ++i) {
            const int v = tid + i * GUM_THREADS;
            if (v < V) {
                const float e = 1.0f / p[i];
                float s = lr[v] * e;
                if (!(s >= GUM_UNDERFLOW)) s = -INFINITY;
                const unsigned long long k = by_rank ? gum_ckey(p[i], v)
                                                     : (unsigned long long)((1 << GUM_IDX_BITS) - 1 - v);
                if (!have || s > bs || (s == bs && k > bk)) { bs = s; bk = k; have = true; }
            }
        }
        if (!have) { bs = -INFINITY; bk = 0; }
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(bs, o);
            const unsigned long long ok = (unsigned long long)__shfl_xor((long long)bk, o);
            if (os > bs || (os == bs && ok > bk)) { bs = os; bk = ok; }
        }
        if ((tid & 63) == 0) { red_f[tid >> 6] = bs; red_k[tid >> 6] = bk; }
        __syncthreads();
        for (int i = 0; i < GUM_WAVES; ++i)
            if (red_f[i] > bs || (red_f[i] == bs && red_k[i] > bk)) { bs = red_f[i]; bk = red_k[i]; }
        token = (1 << GUM_IDX_BITS) - 1 - (long long)(bk & ((1u << GUM_IDX_BITS) - 1));
    }
    if (tid == 0) {
        a.tok_out[b * a.tok_out_stride + step] = token;
        if (a.past_append) a.past_append[b * a.past_stride + t] = token;
    }
}

__global__ void k_gumbel_score(const long long* tokens, long long n, long long L, long long V, const float* key,
                               long long key_row_stride, long long* out_i, float* out_f, int* bad) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long tk = tokens[i];
    float s = 0.f;
    if (tk < 0 || tk >= V) *bad = 1;
    else s = key[(i / L) * key_row_stride + tk];
    if (out_f) out_f[i] = s;
    if (out_i) out_i[i] = (s == INFINITY) ? (long long)0x8000000000000000ull : (long long)s;   // torch's float -> int64 of inf
}

int launch_gumbel_sample(const GumbelArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_gumbel_sample, dim3((unsigned)a.B), dim3(GUM_THREADS), 0, st, a);
    return launch_status("k_gumbel_sample");
}

// ------------------------------------------------------------------ key rows derived on the device (ngram > 0)
// rs = torch.rand(V, generator = CPU MT19937 seeded with hash & 0xffffffff): the generator of keytable.cpp's Mt19937, run by one
// workgroup per hash with its 624-word state in LDS.
//   * seeding s[j] = 1812433253 (s[j-1] ^ s[j-1] >> 30) + j is a dependent chain: one lane walks it (623 steps);
//   * a twist s[k] = s[k+397 mod 624] ^ f(s[k], s[k+1 mod 624]) in ascending k reads NEW words only at distance -227: words 0..226
//     read old state only, 227..453 read the first group's results, 454..623 the second's (and word 623 the new s[0]) -- three
//     parallel phases, each "read, barrier, write, barrier" because word k-1 still needs the old s[k];
//   * tempering and the low 24 bits are per word; the two logarithms are taken in fp64 and rounded to fp32 once, as the host builder
//     (wmar_gumbel_key_build) does: log_rs decides tokens through comparisons of log_rs * (1/p), so the rows must equal the host's bit
//     for bit (tests/test_gpu_gumbel_ctx.py compares 4096 x 16384 entries of all three arrays).
constexpr int MT_N = 624, MT_M = 397;
constexpr int KEY_THREADS = 256;
constexpr int SCORE_THREADS = 64;

__device__ __forceinline__ void mt_seed(uint32_t* s, uint32_t seed) {
    if (threadIdx.x == 0) {
        uint32_t x = seed;
        s[0] = x;
        for (int j = 1; j < MT_N; ++j) { x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)j; s[j] = x; }
    }
    __syncthreads();
}

// every thread of the workgroup (NT of them) calls it; ends behind a barrier
template <int NT>
__device__ __forceinline__ void mt_twist(uint32_t* s) {
    constexpr int PER = (MT_N - MT_M + NT - 1) / NT;      // 227 words in the largest phase
    const int tid = threadIdx.x;
#pragma unroll
    for (int ph = 0; ph < 3; ++ph) {
        const int lo = ph * (MT_N - MT_M), hi = ph == 2 ? MT_N : lo + (MT_N - MT_M);
        uint32_t v[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = lo + tid + i * NT;
            v[i] = 0;
            if (k < hi) {
                const int k1 = k + 1 < MT_N ? k + 1 : 0, km = k + MT_M < MT_N ? k + MT_M : k + MT_M - MT_N;
                const uint32_t y = (s[k] & 0x80000000u) | (s[k1] & 0x7fffffffu);
                v[i] = s[km] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = lo + tid + i * NT;
            if (k < hi) s[k] = v[i];
        }
        __syncthreads();
    }
}

__device__ __forceinline__ float mt_uniform(uint32_t y) {      // at::uniform_real_distribution<float>: 24 bits of the tempered word
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return (float)(y & 0xffffffu) * 5.9604644775390625e-08f;
}
__device__ __forceinline__ float gum_log_rs(float rs) { return (float)log((double)rs); }                  // -inf for rs == 0
__device__ __forceinline__ float gum_score_of(float rs) { return (float)(-log((double)(1.0f - rs))); }

// the three arrays of one hash (any may be null), by the whole workgroup of KEY_THREADS threads
__device__ __forceinline__ void key_row_emit(uint32_t* s, uint32_t seed, int V, float* rs_o, float* lr_o, float* sc_o) {
    mt_seed(s, seed);
    for (int base = 0; base < V; base += MT_N) {
        mt_twist<KEY_THREADS>(s);
        // (the next twist overwrites s only behind its first barrier, i.e. after every thread has left this loop)
        for (int j = threadIdx.x; j < MT_N && base + j < V; j += KEY_THREADS) {
            const float rs = mt_uniform(s[j]);
            if (rs_o) rs_o[base + j] = rs;
            if (lr_o) lr_o[base + j] = gum_log_rs(rs);
            if (sc_o) sc_o[base + j] = gum_score_of(rs);
        }
    }
}

__global__ __launch_bounds__(KEY_THREADS) void k_gumbel_key_rows(const long long* hash, long long V, float* rs, float* lr, float* sc) {
    __shared__ uint32_t s[MT_N];
    const long long b = blockIdx.x;
    const uint32_t seed = (uint32_t)((unsigned long long)hash[b] & 0xffffffffull);      // manual_seed keeps the low 32 bits
    key_row_emit(s, seed, (int)V, rs ? rs + b * V : nullptr, lr ? lr + b * V : nullptr, sc ? sc + b * V : nullptr);
}

// hash of the window in front of position l of one row: h0 ^ ids[l-n] ^ ... ^ ids[l-1]
__device__ __forceinline__ uint32_t ctx_seed(const long long* row, long long l, unsigned long long h0, int n) {
    unsigned long long h = h0;
    for (int i = 0; i < n; ++i) h ^= (unsigned long long)row[l - n + i];
    return (uint32_t)(h & 0xffffffffull);
}

// One decode step of the keyed generation.  Keyed or not is decided on the device-side step counter (workgroup-uniform), so one
// captured graph serves every position of the image.
__global__ __launch_bounds__(KEY_THREADS) void k_gumbel_ctx_keys(GumbelCtxArgs a) {
    __shared__ uint32_t s[MT_N];
    const long long b = blockIdx.x;
    const long long step = *a.step_dev;
    float* out = a.log_rs_out + b * a.V;
    if (step < a.ngram) {
        const float* u = a.u + (step * a.B + b) * a.V;
        for (int v = threadIdx.x; v < (int)a.V; v += KEY_THREADS) out[v] = gum_log_rs(u[v]);
        return;
    }
    key_row_emit(s, ctx_seed(a.ids + b * a.ids_stride, step, a.h0, a.ngram), (int)a.V, nullptr, out, nullptr);
}

// Detector, part 1: which positions are scored.  One workgroup per image, its ids in LDS: position l >= n is scored when no
// earlier position l' >= n carries the same (n+1)-tuple ids[l-n .. l].
__global__ __launch_bounds__(256) void k_gumbel_ctx_mask(const long long* tokens, int L, long long V, int n, signed char* mask,
                                                         int* n_scored, int* bad) {
    extern __shared__ long long tk[];
    __shared__ int cnt;
    const long long b = blockIdx.x;
    if (threadIdx.x == 0) cnt = 0;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        const long long t = tokens[b * L + l];
        if (t < 0 || t >= V) *bad = 1;
        tk[l] = t;
    }
    __syncthreads();
    int mine = 0;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        bool first = l >= n;
        for (int e = n; first && e < l; ++e) {
            bool same = true;
            for (int i = 0; i <= n; ++i) same = same && tk[e - i] == tk[l - i];
            first = !same;
        }
        mask[b * L + l] = first ? 1 : 0;
        mine += first ? 1 : 0;
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0 && n_scored) n_scored[b] = cnt;
}

// Detector, part 2: one wave per position.  Entry ids[b, l] of the window's key needs ids[b, l] / 624 + 1 twists and one logarithm.
__global__ __launch_bounds__(SCORE_THREADS) void k_gumbel_ctx_score(const long long* tokens, long long L, long long V,
                                                                    unsigned long long h0, int n, const signed char* mask,
                                                                    float* scores) {
    __shared__ uint32_t s[MT_N];
    const long long i = blockIdx.x, l = i % L;
    const long long t = tokens[i];
    if (!mask[i] || t < 0 || t >= V) {          // workgroup-uniform
        if (threadIdx.x == 0) scores[i] = 0.f;
        return;
    }
    mt_seed(s, ctx_seed(tokens + (i - l), l, h0, n));
    const int blocks = (int)(t / MT_N) + 1;
    for (int k = 0; k < blocks; ++k) mt_twist<SCORE_THREADS>(s);
    if (threadIdx.x == 0) scores[i] = gum_score_of(mt_uniform(s[t % MT_N]));
}

int launch_gumbel_ctx_keys(const GumbelCtxArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_gumbel_ctx_keys, dim3((unsigned)a.B), dim3(KEY_THREADS), 0, st, a);
    return launch_status("k_gumbel_ctx_keys");
}

}  // namespace wmar

using namespace wmar;

extern "C" {

int wmar_gumbel_sample(const float* logits_dev, int64_t B, int64_t V, const float* log_rs_dev, int64_t key_row_stride,
                       int32_t use_sampling, float temp, float top_p, int32_t top_k, int64_t* tok_out_dev, void* stream) {
    WMAR_REQUIRE(logits_dev && log_rs_dev && tok_out_dev, "gumbel_sample: null argument");
    WMAR_REQUIRE(B >= 0 && V >= 1 && V <= GUM_EPT * GUM_THREADS, "gumbel_sample: vocabulary %lld outside 1..%d", (long long)V,
                 GUM_EPT * GUM_THREADS);
    if (B == 0) return WMAR_OK;
    GumbelArgs a{};
    a.logits = logits_dev; a.V = V; a.B = B; a.log_rs = log_rs_dev; a.key_row_stride = key_row_stride;
    a.use_sampling = use_sampling; a.temp = temp; a.top_p = top_p; a.top_k = top_k;
    a.tok_out = (long long*)tok_out_dev; a.tok_out_stride = 1;
    return launch_gumbel_sample(a, (hipStream_t)stream);
}

int wmar_gumbel_probe_sample(const float* logits_dev, const float* logits_uncond_dev, const float* cfg_scale_dev, int32_t n_steps,
                             const int32_t* step_dev, const int32_t* t_dev, int64_t B, int64_t V, const float* log_rs_dev,
                             int64_t key_row_stride, int32_t use_sampling, float temp, float top_p, int32_t top_k,
                             int64_t* tok_out_dev, int64_t tok_out_stride, int64_t* past_append_dev, int64_t past_stride,
                             void* stream) {
    WMAR_REQUIRE(logits_dev && log_rs_dev && tok_out_dev, "gumbel_probe_sample: null argument");
    WMAR_REQUIRE(B >= 0 && B < (1ll << 31) && V >= 1 && V <= GUM_EPT * GUM_THREADS,
                 "gumbel_probe_sample: vocabulary %lld outside 1..%d", (long long)V, GUM_EPT * GUM_THREADS);
    WMAR_REQUIRE(key_row_stride == 0 || key_row_stride >= V, "gumbel_probe_sample: key rows of stride %lld overlap",
                 (long long)key_row_stride);
    WMAR_REQUIRE(!logits_uncond_dev || cfg_scale_dev, "gumbel_probe_sample: guidance without a scale table");
    WMAR_REQUIRE(n_steps >= 1 && tok_out_stride >= 1 && (!past_append_dev || past_stride >= 1), "gumbel_probe_sample: bad strides");
    if (B == 0) return WMAR_OK;
    hipStream_t st = (hipStream_t)stream;
    // the kernel indexes with what the two counters hold: read them first and refuse a write outside the buffers
    int step = 0, t = 0;
    if (step_dev) WMAR_HIP_CHECK(hipMemcpyAsync(&step, step_dev, sizeof(int), hipMemcpyDeviceToHost, st));
    if (t_dev) WMAR_HIP_CHECK(hipMemcpyAsync(&t, t_dev, sizeof(int), hipMemcpyDeviceToHost, st));
    WMAR_HIP_CHECK(hipStreamSynchronize(st));
    WMAR_REQUIRE(step >= 0 && step < tok_out_stride && (!logits_uncond_dev || step < n_steps),
                 "gumbel_probe_sample: step %d outside the token rows (%lld) or the scale table (%d)", step, (long long)tok_out_stride,
                 n_steps);
    WMAR_REQUIRE(!past_append_dev || (t >= 0 && t < past_stride), "gumbel_probe_sample: length %d outside the id rows (%lld)", t,
                 (long long)past_stride);
    GumbelArgs a{};
    a.logits = logits_dev; a.logits_uncond = logits_uncond_dev; a.cfg_scale = cfg_scale_dev;
    a.step_dev = (const int*)step_dev; a.t_dev = (const int*)t_dev; a.V = V; a.B = B;
    a.log_rs = log_rs_dev; a.key_row_stride = key_row_stride;
    a.use_sampling = use_sampling; a.temp = temp; a.top_p = top_p; a.top_k = top_k;
    a.tok_out = (long long*)tok_out_dev; a.tok_out_stride = tok_out_stride;
    a.past_append = (long long*)past_append_dev; a.past_stride = past_stride;
    int rc = launch_gumbel_sample(a, st);
    if (rc) return rc;
    WMAR_HIP_CHECK(hipStreamSynchronize(st));
    return WMAR_OK;
}

int wmar_gumbel_score(const int64_t* tokens_dev, int64_t B, int64_t L, int64_t V, const float* score_key_dev,
                      int64_t key_row_stride, int64_t* scores_i64_dev, float* scores_f32_dev, void* stream) {
    WMAR_REQUIRE(tokens_dev && score_key_dev, "gumbel_score: null argument");
    WMAR_REQUIRE(B >= 0 && L >= 1 && V >= 1, "gumbel_score: bad shape");
    if (B == 0) return WMAR_OK;
    hipStream_t st = (hipStream_t)stream;
    int* bad = nullptr;
    WMAR_HIP_CHECK(hipMalloc(&bad, sizeof(int)));
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int), st);
    const long long n = B * L;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_gumbel_score, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const long long*)tokens_dev, n,
                           (long long)L, (long long)V, score_key_dev, (long long)key_row_stride, (long long*)scores_i64_dev,
                           scores_f32_dev, bad);
        e = hipGetLastError();
    }
    int hbad = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(bad);
    if (e != hipSuccess) { set_error("gumbel_score: %s", hipGetErrorString(e)); return WMAR_EHIP; }
    WMAR_REQUIRE(!hbad, "gumbel_score: token id outside [0, %lld)", (long long)V);
    return WMAR_OK;
}

int wmar_gumbel_key_rows(const int64_t* hash_dev, int64_t N, int64_t V, float* rs_out_dev, float* log_rs_out_dev,
                         float* score_out_dev, void* stream) {
    WMAR_REQUIRE(hash_dev || N == 0, "gumbel_key_rows: null argument");
    WMAR_REQUIRE(N >= 0 && N < (1ll << 31) && V >= 1 && V < (1ll << 31), "gumbel_key_rows: bad shape");
    if (N == 0 || !(rs_out_dev || log_rs_out_dev || score_out_dev)) return WMAR_OK;
    hipLaunchKernelGGL(k_gumbel_key_rows, dim3((unsigned)N), dim3(KEY_THREADS), 0, (hipStream_t)stream, (const long long*)hash_dev,
                       (long long)V, rs_out_dev, log_rs_out_dev, score_out_dev);
    return launch_status("k_gumbel_key_rows");
}

int wmar_gumbel_score_ctx(const int64_t* tokens_dev, int64_t B, int64_t L, int64_t V, uint64_t h0, int32_t ngram,
                          float* scores_f32_dev, int8_t* scored_mask_dev, int32_t* n_scored_dev, void* stream) {
    WMAR_REQUIRE(tokens_dev && scores_f32_dev && scored_mask_dev, "gumbel_score_ctx: null argument");
    WMAR_REQUIRE(ngram >= 1 && ngram <= WMAR_MAX_CONTEXT, "gumbel_score_ctx: ngram %d outside 1..%d", ngram, WMAR_MAX_CONTEXT);
    WMAR_REQUIRE(B >= 0 && B < (1ll << 31) && V >= 1 && V <= GUM_EPT * GUM_THREADS, "gumbel_score_ctx: bad shape");
    if (L <= ngram) {
        set_error("gumbel_score_ctx: %lld codes leave nothing to score behind a window of %d", (long long)L, ngram);
        return WMAR_ESHORT;
    }
    WMAR_REQUIRE(L <= 4096 && B * L < (1ll << 31), "gumbel_score_ctx: passage of %lld codes too long (4096)", (long long)L);
    if (B == 0) return WMAR_OK;
    hipStream_t st = (hipStream_t)stream;
    int* bad = nullptr;
    WMAR_HIP_CHECK(hipMalloc(&bad, sizeof(int)));
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_gumbel_ctx_mask, dim3((unsigned)B), dim3(256), (size_t)L * sizeof(long long), st,
                           (const long long*)tokens_dev, (int)L, (long long)V, (int)ngram, (signed char*)scored_mask_dev,
                           (int*)n_scored_dev, bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_gumbel_ctx_score, dim3((unsigned)(B * L)), dim3(SCORE_THREADS), 0, st, (const long long*)tokens_dev,
                           (long long)L, (long long)V, (unsigned long long)h0, (int)ngram, (const signed char*)scored_mask_dev,
                           scores_f32_dev);
        e = hipGetLastError();
    }
    int hbad = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(bad);
    if (e != hipSuccess) { set_error("gumbel_score_ctx: %s", hipGetErrorString(e)); return WMAR_EHIP; }
    WMAR_REQUIRE(!hbad, "gumbel_score_ctx: token id outside [0, %lld)", (long long)V);
    return WMAR_OK;
}

}  // extern "C"
