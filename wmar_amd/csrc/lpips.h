// LPIPS on the device (gfx950): the perceptual term of the tokenizer fine-tuning loss -- a frozen VGG16 on two images, the LPIPS head on
// five feature taps, and the gradient towards the first image.  Included at the end of vqgan.hip behind vq_train.h: it shares that
// translation unit's run_conv, Loader, DeviceArena and k_flip_transpose_w, and adds no dispatch rule and no instantiation to them.
//
// Reference: deps/taming/modules/losses/lpips.py:41-122 in .eval() (dropout inactive) under torch.autograd, as
// deps/taming/modules/losses/vqperceptual.py:83-92 and deps/rar/modeling/titok.py:113-115 call it.
//
//   scaling   (x - shift) / scale per channel, NCHW [B, 3, S, S] -> NHWC with 8 stored channels (k_lpips_input); backward g / scale.
//   VGG16     features[0:30]: thirteen 3 x 3 convs with bias (run_conv), each followed by ReLU, in slices of 2, 2, 3, 3, 3 convs; a
//             2 x 2 stride-2 max-pool in front of slices 2..5.  The five slice outputs are the taps.
//   head      per tap: n = f / (sqrt(sum_c f^2) + 1e-10) for both images, sum_c w_c (n0_c - n1_c)^2, spatial mean; the five taps are
//             added in the order 0..4.
//
// Conventions are vq_grad.h's: activations NHWC fp32 (every slice width is a multiple of 8, so only the image has padding channels), no
// floating-point atomics, every reduction in a fixed order, all memory allocated at create time for max_batch images.
//
//   ReLU      y = x < 0 ? 0 : x -- x > 0 ? x : 0 everywhere except that -0.0 stays -0.0 and a NaN stays a NaN, which is what torch's
//             relu (clamp_min) returns; in place behind the conv (k_relu), or fused with the pool that follows it (k_relu_pool: one pass
//             writes the tap and the pooled tensor).  Backward: g where the taped y > 0, else 0.
//   max-pool  backward: the whole gradient goes to the FIRST maximum of the window in row-major order (torch's rule: a later element
//             replaces the maximum only when it is strictly greater).  k_relu_pool_bwd fuses it with the add of the tap's gradient and
//             with the ReLU mask.
//   head      per-pixel channel sums (sum f^2, sum w d^2, sum a f) in fp64: per lane in channel order, then a fixed butterfly over the
//             wave.  The spatial mean is a two-stage sum of fp64 partials (per wave in pixel order, per workgroup, then in chunk order).
//             At a pixel whose feature vector is all zero the gradient is 0: torch ends there too (its sqrt backward makes a NaN that
//             the ReLU mask behind it replaces by 0).
//   dgrad     every conv is stride 1: run_conv on the flipped, transposed weight, packed once at create time (the weights are frozen;
//             there is no weight gradient anywhere).
//
// Tape: the thirteen post-ReLU activations of the `input` branch (ReLU masks, pool windows, head) and the five normalised taps of the
// `target` branch.  The target branch itself runs in two ping-pong buffers, which the backward reuses for the gradients.
#pragma once

namespace wmar {

constexpr int LP_MAXQ = 4;              // float4 per lane and pixel in the head kernels: at most 1024 channels
constexpr int LP_CHUNKS_MAX = 256;      // spatial chunks (workgroups) per image in the head kernels

__device__ __forceinline__ float lp_relu(float x) { return x < 0.0f ? 0.0f : x; }
__device__ __forceinline__ float4 lp_relu4(float4 v) { return make_float4(lp_relu(v.x), lp_relu(v.y), lp_relu(v.z), lp_relu(v.w)); }
__device__ __forceinline__ double lp_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// x [B][3][HW] -> y [B][HW][8] = (x - shift) / scale: an fp32 subtract, then an fp32 divide; padding channels 0
__global__ void k_lpips_input(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ shift,
                              const float* __restrict__ scale, int HW) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long b = blockIdx.y;
    if (idx >= HW) return;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float d = x[(b * 3 + c) * HW + idx] - shift[c];
        v[c] = d / scale[c];
    }
    float4* o = (float4*)(y + (b * HW + idx) * 8);
    o[0] = make_float4(v[0], v[1], v[2], 0.0f);
    o[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// g [B][HW][8] -> out [B][3][HW] = g / scale
__global__ void k_lpips_input_bwd(const float* __restrict__ g, float* __restrict__ out, const float* __restrict__ scale, int HW) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long b = blockIdx.y;
    if (idx >= HW) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(b * 3 + c) * HW + idx] = g[(b * HW + idx) * 8 + c] / scale[c];
}

// y = relu(x); x and y may be the same buffer
__global__ void k_relu(const float* x, float* y, long long n4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    ((float4*)y)[i] = lp_relu4(((const float4*)x)[i]);
}

// gx = g where the taped y > 0, else 0; g and gx may be the same buffer
__global__ void k_relu_bwd(const float* __restrict__ y, const float* g, float* gx, long long n4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4 yv = ((const float4*)y)[i], gv = ((const float4*)g)[i];
    ((float4*)gx)[i] = make_float4(yv.x > 0.0f ? gv.x : 0.0f, yv.y > 0.0f ? gv.y : 0.0f, yv.z > 0.0f ? gv.z : 0.0f, yv.w > 0.0f ? gv.w : 0.0f);
}

// x [B][2Ho][2Wo][C] -> y = relu(x) (may be x itself) and p [B][Ho][Wo][C] = the maximum of each 2 x 2 window of y, scanned top-left,
// top-right, bottom-left, bottom-right with a strict comparison.  One thread per (pooled pixel, four channels).
__global__ void k_relu_pool(const float* x, float* y, float* __restrict__ p, long long total, int Ho, int Wo, int C) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int q4 = C >> 2;
    const int c = (int)(idx % q4) * 4;
    const long long pix = idx / q4;
    const int ox = (int)(pix % Wo);
    const long long t = pix / Wo;
    const int oy = (int)(t % Ho);
    const long long b = t / Ho;
    const long long row = 2LL * Wo * C;
    const long long o00 = ((b * 2 * Ho + 2 * oy) * (2LL * Wo) + 2 * ox) * C + c;
    const long long offs[4] = {o00, o00 + C, o00 + row, o00 + row + C};
    float4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = lp_relu4(*(const float4*)(x + offs[i]));
    float4 m = v[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        if (v[i].x > m.x) m.x = v[i].x;
        if (v[i].y > m.y) m.y = v[i].y;
        if (v[i].z > m.z) m.z = v[i].z;
        if (v[i].w > m.w) m.w = v[i].w;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) *(float4*)(y + offs[i]) = v[i];
    *(float4*)(p + pix * C + c) = m;
}

// Backward of k_relu_pool at the taped y [B][2Ho][2Wo][C]: gp [B][Ho][Wo][C] goes to the first maximum of its window, gt (the gradient
// that reaches y directly, from the tap's head; may be null) is added, and the sum passes where y > 0.  gx may be gt itself.
__global__ void k_relu_pool_bwd(const float* __restrict__ y, const float* __restrict__ gp, const float* gt, float* gx, long long total, int Ho,
                                int Wo, int C) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int q4 = C >> 2;
    const int c = (int)(idx % q4) * 4;
    const long long pix = idx / q4;
    const int ox = (int)(pix % Wo);
    const long long t = pix / Wo;
    const int oy = (int)(t % Ho);
    const long long b = t / Ho;
    const long long row = 2LL * Wo * C;
    const long long o00 = ((b * 2 * Ho + 2 * oy) * (2LL * Wo) + 2 * ox) * C + c;
    const long long offs[4] = {o00, o00 + C, o00 + row, o00 + row + C};
    float yv[4][4], tv[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 a = *(const float4*)(y + offs[i]);
        yv[i][0] = a.x; yv[i][1] = a.y; yv[i][2] = a.z; yv[i][3] = a.w;
        float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gt) g = *(const float4*)(gt + offs[i]);
        tv[i][0] = g.x; tv[i][1] = g.y; tv[i][2] = g.z; tv[i][3] = g.w;
    }
    const float4 g4 = *(const float4*)(gp + pix * C + c);
    const float gpv[4] = {g4.x, g4.y, g4.z, g4.w};
    float o[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int first = 0;
        float m = yv[0][k];
#pragma unroll
        for (int i = 1; i < 4; ++i)
            if (yv[i][k] > m) { m = yv[i][k]; first = i; }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float routed = i == first ? gpv[k] : 0.0f;
            const float s = gt ? routed + tv[i][k] : routed;
            o[i][k] = yv[i][k] > 0.0f ? s : 0.0f;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) *(float4*)(gx + offs[i]) = make_float4(o[i][0], o[i][1], o[i][2], o[i][3]);
}

// the lane's channels of one pixel: quads lane, lane + 64, ... (the same assignment in every head kernel)
__device__ __forceinline__ double lp_load_sq(const float* __restrict__ f, int C, int lane, float4 (&v)[LP_MAXQ]) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < LP_MAXQ; ++i) {
        const int c = (lane + 64 * i) * 4;
        v[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (c < C) { v[i] = *(const float4*)(f + c); s += sq4_f64(v[i]); }
    }
    return lp_wave_sum(s);
}

// n = f / (sqrt(sum_c f^2) + 1e-10) per pixel (normalize_tensor): one wave per pixel
__global__ __launch_bounds__(256) void k_lpips_normalize(const float* __restrict__ f, float* __restrict__ n, long long npix, int C) {
    const long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= npix) return;
    const int lane = threadIdx.x & 63;
    float4 v[LP_MAXQ];
    const double s = lp_load_sq(f + pix * C, C, lane, v);
    const float den = sqrtf((float)s) + 1e-10f;
#pragma unroll
    for (int i = 0; i < LP_MAXQ; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < C) *(float4*)(n + pix * C + c) = make_float4(v[i].x / den, v[i].y / den, v[i].z / den, v[i].w / den);
    }
}

struct LpHeadArgs {
    const float* f0;     // [B][HW][C]: the tap of the first image (post-ReLU)
    const float* n1;     // [B][HW][C]: the normalised tap of the second image
    const float* w;      // [C]: the tap's lin weight
    double* part;        // [B][nchunk]: per-chunk sums of the per-pixel values
    const float* gv;     // [B]: gradient of the tap's value (backward)
    float* g0;           // [B][HW][C]: gradient towards f0 (backward)
    int HW, C, nchunk;
};

// per (image, chunk): the sum over the chunk's pixels of sum_c w_c (n0_c - n1_c)^2.  Wave w of the workgroup takes the pixels
// p0 + w, p0 + w + 4, ... in order; the four waves' sums are added in wave order.
__global__ __launch_bounds__(256) void k_lpips_head_fwd(LpHeadArgs a) {
    __shared__ double red[4];
    const int b = blockIdx.y, chunk = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p0 = (int)((long long)chunk * a.HW / a.nchunk), p1 = (int)((long long)(chunk + 1) * a.HW / a.nchunk);
    double acc = 0.0;
    for (int p = p0 + wave; p < p1; p += 4) {
        const long long off = ((long long)b * a.HW + p) * a.C;
        float4 v[LP_MAXQ];
        const double s = lp_load_sq(a.f0 + off, a.C, lane, v);
        const float den = sqrtf((float)s) + 1e-10f;
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < LP_MAXQ; ++i) {
            const int c = (lane + 64 * i) * 4;
            if (c < a.C) {
                const float4 n = *(const float4*)(a.n1 + off + c), w = *(const float4*)(a.w + c);
                const float fs[4] = {v[i].x, v[i].y, v[i].z, v[i].w}, ns[4] = {n.x, n.y, n.z, n.w}, ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float d = fs[k] / den - ns[k];
                    t += prod_f64(ws[k], d * d);
                }
            }
        }
        acc += lp_wave_sum(t);
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) a.part[(long long)b * a.nchunk + chunk] = ((red[0] + red[1]) + red[2]) + red[3];
}

// out[b] = (part[b][0] + part[b][1] + ...) / HW
__global__ void k_lpips_head_fold(const double* __restrict__ part, float* __restrict__ out, int B, int nchunk, int HW) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double t = 0.0;
    for (int k = 0; k < nchunk; ++k) t += part[(long long)b * nchunk + k];
    double m = t * inv_count_f64((double)HW);
    asm volatile("" : "+v"(m));
    out[b] = (float)m;
}

// value[b] = taps[0][b] + taps[1][b] + ... + taps[4][b] (fp32, tap order); per_tap [5][B] gets a copy when it is not null
__global__ void k_lpips_total(const float* __restrict__ taps, int tstride, float* __restrict__ value, float* __restrict__ per_tap, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float v = taps[b];
    for (int k = 1; k < 5; ++k) v += taps[k * tstride + b];
    value[b] = v;
    if (per_tap)
        for (int k = 0; k < 5; ++k) per_tap[k * B + b] = taps[k * tstride + b];
}

// g0 = d value / d f0 * gv[b]: with r = |f0|, n0 = f0 / (r + eps), a_c = 2 w_c (n0_c - n1_c) and gs = gv[b] / HW,
// g0_j = gs (a_j / (r + eps) - f0_j (sum_c a_c f0_c) / ((r + eps)^2 r)), and 0 at a pixel with r = 0.
__global__ __launch_bounds__(256) void k_lpips_head_bwd(LpHeadArgs a) {
    const int b = blockIdx.y, chunk = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p0 = (int)((long long)chunk * a.HW / a.nchunk), p1 = (int)((long long)(chunk + 1) * a.HW / a.nchunk);
    const float gs = a.gv[b] / (float)a.HW;
    for (int p = p0 + wave; p < p1; p += 4) {
        const long long off = ((long long)b * a.HW + p) * a.C;
        float4 v[LP_MAXQ];
        const double s = lp_load_sq(a.f0 + off, a.C, lane, v);
        const float r = sqrtf((float)s);
        if (r == 0.0f) {                        // the same for the whole wave: s is the wave's sum
#pragma unroll
            for (int i = 0; i < LP_MAXQ; ++i) {
                const int c = (lane + 64 * i) * 4;
                if (c < a.C) *(float4*)(a.g0 + off + c) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            continue;
        }
        const float den = r + 1e-10f, inv = 1.0f / den;
        float av[LP_MAXQ][4];
        double dot = 0.0;
#pragma unroll
        for (int i = 0; i < LP_MAXQ; ++i) {
            const int c = (lane + 64 * i) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) av[i][k] = 0.0f;
            if (c < a.C) {
                const float4 n = *(const float4*)(a.n1 + off + c), w = *(const float4*)(a.w + c);
                const float fs[4] = {v[i].x, v[i].y, v[i].z, v[i].w}, ns[4] = {n.x, n.y, n.z, n.w}, ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    av[i][k] = 2.0f * ws[k] * (fs[k] / den - ns[k]);
                    dot += prod_f64(av[i][k], fs[k]);
                }
            }
        }
        dot = lp_wave_sum(dot);
        const float kf = (float)dot * inv * inv / r;
#pragma unroll
        for (int i = 0; i < LP_MAXQ; ++i) {
            const int c = (lane + 64 * i) * 4;
            if (c < a.C) {
                const float fs[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = gs * (av[i][k] * inv - fs[k] * kf);
                *(float4*)(a.g0 + off + c) = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
    }
}

}  // namespace wmar

namespace {

constexpr int LP_CONVS = 13;
constexpr int LP_SLICE_CONVS[5] = {2, 2, 3, 3, 3};
constexpr int LP_VGG_INDEX[LP_CONVS] = {0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28};      // torchvision's features[N]

struct LpConv { ConvW fw, dg; };

inline unsigned lp_grid(long long n) { return (unsigned)((n + 255) / 256); }
inline int lp_chunks(int HW) { int n = HW / 64; return n < 1 ? 1 : (n > LP_CHUNKS_MAX ? LP_CHUNKS_MAX : n); }

int run_lpips_input(const float* x, float* y, const float* shift, const float* scale, int B, int HW, hipStream_t st) {
    hipLaunchKernelGGL(k_lpips_input, dim3((HW + 255) / 256, (unsigned)B), dim3(256), 0, st, x, y, shift, scale, HW);
    return launch_status("k_lpips_input");
}
int run_lpips_input_backward(const float* g, float* out, const float* scale, int B, int HW, hipStream_t st) {
    hipLaunchKernelGGL(k_lpips_input_bwd, dim3((HW + 255) / 256, (unsigned)B), dim3(256), 0, st, g, out, scale, HW);
    return launch_status("k_lpips_input_bwd");
}
// x [B][H][W][C] -> y = relu(x) (in place when y == x); p [B][H/2][W/2][C] the pooled tensor, or null for the ReLU alone
int run_relu_pool(const float* x, float* y, float* p, int B, int H, int W, int C, hipStream_t st) {
    WMAR_REQUIRE(C % 4 == 0, "ReLU: channel count %d is not a multiple of 4", C);
    if (!p) {
        const long long n4 = (long long)B * H * W * (C / 4);
        hipLaunchKernelGGL(k_relu, dim3(lp_grid(n4)), dim3(256), 0, st, x, y, n4);
        return launch_status("k_relu");
    }
    WMAR_REQUIRE(H % 2 == 0 && W % 2 == 0, "max-pool: %d x %d is not even", H, W);
    const long long total = (long long)B * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(k_relu_pool, dim3(lp_grid(total)), dim3(256), 0, st, x, y, p, total, H / 2, W / 2, C);
    return launch_status("k_relu_pool");
}
// y [B][H][W][C] taped; gp [B][H/2][W/2][C] or null (no pool behind this ReLU: gt is the gradient); gx may be gt
int run_relu_pool_backward(const float* y, const float* gp, const float* gt, float* gx, int B, int H, int W, int C, hipStream_t st) {
    WMAR_REQUIRE(C % 4 == 0, "ReLU backward: channel count %d is not a multiple of 4", C);
    if (!gp) {
        WMAR_REQUIRE(gt, "ReLU backward: no gradient");
        const long long n4 = (long long)B * H * W * (C / 4);
        hipLaunchKernelGGL(k_relu_bwd, dim3(lp_grid(n4)), dim3(256), 0, st, y, gt, gx, n4);
        return launch_status("k_relu_bwd");
    }
    WMAR_REQUIRE(H % 2 == 0 && W % 2 == 0, "max-pool backward: %d x %d is not even", H, W);
    const long long total = (long long)B * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(k_relu_pool_bwd, dim3(lp_grid(total)), dim3(256), 0, st, y, gp, gt, gx, total, H / 2, W / 2, C);
    return launch_status("k_relu_pool_bwd");
}
int run_lpips_normalize(const float* f, float* n, int B, int HW, int C, hipStream_t st) {
    WMAR_REQUIRE(C % 4 == 0 && C <= 256 * LP_MAXQ, "LPIPS head: channel count %d unsupported (multiple of 4, <= %d)", C, 256 * LP_MAXQ);
    const long long npix = (long long)B * HW;
    hipLaunchKernelGGL(k_lpips_normalize, dim3((unsigned)((npix + 3) / 4)), dim3(256), 0, st, f, n, npix, C);
    return launch_status("k_lpips_normalize");
}
// doubles of scratch run_lpips_head needs
inline size_t lpips_head_doubles(int B, int HW) { return (size_t)B * lp_chunks(HW); }
// value[b] = mean over pixels of sum_c w_c (n0_c - n1_c)^2 with n0 the normalised f0
int run_lpips_head(const float* f0, const float* n1, const float* w, double* part, float* value, int B, int HW, int C, hipStream_t st) {
    WMAR_REQUIRE(C % 4 == 0 && C <= 256 * LP_MAXQ, "LPIPS head: channel count %d unsupported (multiple of 4, <= %d)", C, 256 * LP_MAXQ);
    LpHeadArgs a{};
    a.f0 = f0; a.n1 = n1; a.w = w; a.part = part; a.HW = HW; a.C = C; a.nchunk = lp_chunks(HW);
    hipLaunchKernelGGL(k_lpips_head_fwd, dim3(a.nchunk, (unsigned)B), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_lpips_head_fold, dim3((B + 63) / 64), dim3(64), 0, st, (const double*)part, value, B, a.nchunk, HW);
    return launch_status("k_lpips_head_fwd");
}
int run_lpips_head_backward(const float* f0, const float* n1, const float* w, const float* gv, float* g0, int B, int HW, int C, hipStream_t st) {
    WMAR_REQUIRE(C % 4 == 0 && C <= 256 * LP_MAXQ, "LPIPS head: channel count %d unsupported (multiple of 4, <= %d)", C, 256 * LP_MAXQ);
    LpHeadArgs a{};
    a.f0 = f0; a.n1 = n1; a.w = w; a.gv = gv; a.g0 = g0; a.HW = HW; a.C = C; a.nchunk = lp_chunks(HW);
    hipLaunchKernelGGL(k_lpips_head_bwd, dim3(a.nchunk, (unsigned)B), dim3(256), 0, st, a);
    return launch_status("k_lpips_head_bwd");
}

}  // namespace

struct wmar_lpips {
    DeviceArena mem;
    int chns[5] = {0, 0, 0, 0, 0};
    int S = 0, Bmax = 0;
    LpConv convs[LP_CONVS];
    float* lin[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float *shift = nullptr, *scale = nullptr;
    // the tape: post-ReLU activations of the input branch, normalised taps of the target branch
    float* y[LP_CONVS] = {};
    float* tn[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // scratch: the scaled image, two activation-sized buffers (target branch, pooled tensors, gradients), the head's partial sums, the taps
    float *xin = nullptr, *buf[2] = {nullptr, nullptr}, *taps = nullptr;
    double* part = nullptr;
    bool tape = false;
    int tapeB = 0;
};

namespace {

// One branch of the forward.  input_branch: the convs write the tape and every tap runs the head against tn[k] (taps[k][b]); else the
// convs run in the two scratch buffers and every tap is normalised into tn[k].
int lpips_branch(wmar_lpips* e, const float* img, int B, bool input_branch, hipStream_t st) {
    int rc;
    if ((rc = run_lpips_input(img, e->xin, e->shift, e->scale, B, e->S * e->S, st))) return rc;
    const float* in = e->xin;
    int ci = 0;
    for (int k = 0; k < 5; ++k) {
        const int H = e->S >> k, C = e->chns[k];
        float* out = nullptr;
        for (int j = 0; j < LP_SLICE_CONVS[k]; ++j, ++ci) {
            out = input_branch ? e->y[ci] : (in == e->buf[0] ? e->buf[1] : e->buf[0]);
            if ((rc = run_conv(e->convs[ci].fw, in, out, nullptr, B, H, H, 1, 0, st))) return rc;
            const bool pool = j == LP_SLICE_CONVS[k] - 1 && k < 4;
            float* pooled = pool ? (input_branch || out == e->buf[1] ? e->buf[0] : e->buf[1]) : nullptr;
            if ((rc = run_relu_pool(out, out, pooled, B, H, H, C, st))) return rc;
            in = pool ? pooled : out;
        }
        if (input_branch) {
            if ((rc = run_lpips_head(out, e->tn[k], e->lin[k], e->part, e->taps + (size_t)k * e->Bmax, B, H * H, C, st))) return rc;
        } else {
            if ((rc = run_lpips_normalize(out, e->tn[k], B, H * H, C, st))) return rc;
        }
    }
    return WMAR_OK;
}

}  // namespace

extern "C" {

int wmar_lpips_create(const wmar_lpips_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream,
                      wmar_lpips** out) {
    WMAR_REQUIRE(cfg && names && tensors_dev && out, "lpips_create: null argument");
    WMAR_REQUIRE(cfg->resolution >= 128 && cfg->resolution <= 1024 && cfg->resolution % 128 == 0,
                 "lpips_create: resolution %d is not a multiple of 128 in 128..1024 (relu5_3 is resolution / 16 and the convolutions work on "
                 "8 x 8 tiles)", cfg->resolution);
    WMAR_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= 64, "lpips_create: max_batch %d outside 1..64", cfg->max_batch);
    for (int k = 0; k < 5; ++k)
        WMAR_REQUIRE(cfg->chns[k] >= 8 && cfg->chns[k] <= 256 * LP_MAXQ && cfg->chns[k] % 8 == 0,
                     "lpips_create: slice width %d (slice %d) is not a multiple of 8 in 8..%d", cfg->chns[k], k + 1, 256 * LP_MAXQ);
    std::unique_ptr<wmar_lpips> e(new wmar_lpips());
    e->S = cfg->resolution; e->Bmax = cfg->max_batch;
    for (int k = 0; k < 5; ++k) e->chns[k] = cfg->chns[k];
    hipStream_t st = (hipStream_t)stream;
    const int S = e->S, Bmax = e->Bmax;
    DeviceArena tmp;                    // the flipped weights: read by the packers only, released when create returns
    Loader ld(names, tensors_dev, n_tensors, &e->mem, st);
    int& rc = ld.rc;
    const float* sh = ld.need("scaling_layer.shift");
    const float* sc = ld.need("scaling_layer.scale");
    WMAR_TRY(e->mem.alloc(&e->shift, 4));
    WMAR_TRY(e->mem.alloc(&e->scale, 4));
    if (rc == WMAR_OK && (hipMemcpyAsync(e->shift, sh, 12, hipMemcpyDeviceToDevice, st) != hipSuccess ||
                          hipMemcpyAsync(e->scale, sc, 12, hipMemcpyDeviceToDevice, st) != hipSuccess)) {
        set_error("lpips_create: copy of the scaling constants failed"); rc = WMAR_EHIP;
    }
    size_t act_elems = 0;
    int ci = 0, cin = 3;
    for (int k = 0; k < 5 && rc == WMAR_OK; ++k) {
        const int H = S >> k, C = e->chns[k];
        act_elems = std::max(act_elems, (size_t)H * H * C);
        for (int j = 0; j < LP_SLICE_CONVS[k] && rc == WMAR_OK; ++j, ++ci) {
            char name[64];
            snprintf(name, sizeof name, "net.slice%d.%d", k + 1, LP_VGG_INDEX[ci]);
            LpConv& c = e->convs[ci];
            ld.conv(name, cin, C, 3, c.fw, true);
            if (rc != WMAR_OK) break;
            const float* W = ld.need(std::string(name) + ".weight");
            const size_t nw = (size_t)C * cin * 9;
            float* wt = nullptr;
            WMAR_TRY(tmp.alloc(&wt, nw));
            if (rc == WMAR_OK) {
                hipLaunchKernelGGL(k_flip_transpose_w, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, W, wt, C, cin, 3);
                const char* dnames[1] = {"dgrad.weight"};
                const void* dtensors[1] = {wt};
                Loader l2(dnames, dtensors, 1, &e->mem, st);
                l2.conv("dgrad", C, cin, 3, c.dg, false);
                rc = l2.rc;
            }
            WMAR_TRY(e->mem.alloc(&e->y[ci], (size_t)Bmax * H * H * C));
            cin = C;
        }
        if (rc != WMAR_OK) break;
        char name[64];
        snprintf(name, sizeof name, "lin%d.model.1.weight", k);
        const float* lw = ld.need(name);
        WMAR_TRY(e->mem.alloc(&e->lin[k], (size_t)C));
        if (rc == WMAR_OK && hipMemcpyAsync(e->lin[k], lw, (size_t)C * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            set_error("lpips_create: copy of %s failed", name); rc = WMAR_EHIP;
        }
        WMAR_TRY(e->mem.alloc(&e->tn[k], (size_t)Bmax * H * H * C));
    }
    WMAR_TRY(e->mem.alloc(&e->xin, (size_t)Bmax * S * S * 8));
    WMAR_TRY(e->mem.alloc(&e->buf[0], (size_t)Bmax * act_elems));
    WMAR_TRY(e->mem.alloc(&e->buf[1], (size_t)Bmax * act_elems));
    WMAR_TRY(e->mem.alloc(&e->taps, (size_t)5 * Bmax));
    WMAR_TRY(e->mem.alloc(&e->part, lpips_head_doubles(Bmax, S * S)));
    const hipError_t se = hipStreamSynchronize(st);
    if (rc == WMAR_OK && se != hipSuccess) { set_error("lpips_create: sync failed: %s", hipGetErrorString(se)); rc = WMAR_EHIP; }
    if (rc != WMAR_OK) return rc;
    *out = e.release();
    return WMAR_OK;
}

void wmar_lpips_destroy(wmar_lpips* e) { delete e; }
int64_t wmar_lpips_device_bytes(const wmar_lpips* e) { return e ? e->mem.bytes : 0; }

int wmar_lpips_forward(wmar_lpips* e, const float* input_dev, const float* target_dev, int64_t B, int32_t keep_tape, float* value_dev,
                       float* per_tap_dev, void* stream) {
    WMAR_REQUIRE(e && input_dev && target_dev && value_dev, "lpips_forward: null argument");
    WMAR_REQUIRE(B >= 1 && B <= e->Bmax, "lpips_forward: batch %lld outside 1..%d", (long long)B, e->Bmax);
    hipStream_t st = (hipStream_t)stream;
    e->tape = false;
    g_trk = GnTrack{};
    if (int rc = lpips_branch(e, target_dev, (int)B, false, st)) return rc;
    if (int rc = lpips_branch(e, input_dev, (int)B, true, st)) return rc;
    hipLaunchKernelGGL(k_lpips_total, dim3(((int)B + 63) / 64), dim3(64), 0, st, (const float*)e->taps, e->Bmax, value_dev, per_tap_dev, (int)B);
    if (int rc = launch_status("k_lpips_total")) return rc;
    e->tape = keep_tape != 0;
    e->tapeB = (int)B;
    return WMAR_OK;
}

int wmar_lpips_backward(wmar_lpips* e, const float* grad_value_dev, int64_t B, float* grad_input_dev, void* stream) {
    WMAR_REQUIRE(e && grad_value_dev && grad_input_dev, "lpips_backward: null argument");
    WMAR_REQUIRE(e->tape, "lpips_backward: no tape (the last wmar_lpips_forward did not keep one, or there was none)");
    WMAR_REQUIRE(B == e->tapeB, "lpips_backward: batch %lld, the tape holds %d", (long long)B, e->tapeB);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    g_trk = GnTrack{};
    const int Bi = (int)B;
    float* cur = nullptr;               // gradient of the pooled tensor the slice below handed up
    int ci = LP_CONVS - 1;
    for (int k = 4; k >= 0; --k) {
        const int H = e->S >> k, C = e->chns[k];
        float* t = cur == e->buf[0] ? e->buf[1] : e->buf[0];
        if ((rc = run_lpips_head_backward(e->y[ci], e->tn[k], e->lin[k], grad_value_dev, t, Bi, H * H, C, st))) return rc;
        if ((rc = run_relu_pool_backward(e->y[ci], cur, t, t, Bi, H, H, C, st))) return rc;
        float* src = t;
        for (int j = LP_SLICE_CONVS[k] - 1; j >= 0; --j, --ci) {
            float* dst = src == e->buf[0] ? e->buf[1] : e->buf[0];
            if ((rc = run_conv(e->convs[ci].dg, src, dst, nullptr, Bi, H, H, 1, 0, st))) return rc;
            if (j > 0 && (rc = run_relu_pool_backward(e->y[ci - 1], nullptr, dst, dst, Bi, H, H, C, st))) return rc;
            src = dst;
        }
        cur = src;
    }
    return run_lpips_input_backward(cur, grad_input_dev, e->scale, Bi, e->S * e->S, st);
}

// ------------------------------------------------------------------------------ probes (tests): one new layer alone
int wmar_lpips_probe_input(const float* x_dev, const float* shift_dev, const float* scale_dev, int64_t B, int32_t HW, float* y_dev, void* stream) {
    WMAR_REQUIRE(x_dev && shift_dev && scale_dev && y_dev, "lpips_probe_input: null argument");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && HW >= 1, "lpips_probe_input: bad shape");
    hipStream_t st = (hipStream_t)stream;
    return probe_finish(run_lpips_input(x_dev, y_dev, shift_dev, scale_dev, (int)B, HW, st), st);
}

int wmar_lpips_probe_input_backward(const float* g_nhwc_dev, const float* scale_dev, int64_t B, int32_t HW, float* g_nchw_dev, void* stream) {
    WMAR_REQUIRE(g_nhwc_dev && scale_dev && g_nchw_dev, "lpips_probe_input_backward: null argument");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && HW >= 1, "lpips_probe_input_backward: bad shape");
    hipStream_t st = (hipStream_t)stream;
    return probe_finish(run_lpips_input_backward(g_nhwc_dev, g_nchw_dev, scale_dev, (int)B, HW, st), st);
}

int wmar_lpips_probe_relu_pool(const float* x_dev, int64_t B, int32_t H, int32_t W, int32_t C, float* y_dev, float* p_dev, void* stream) {
    WMAR_REQUIRE(x_dev && y_dev, "lpips_probe_relu_pool: null argument");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && H >= 1 && W >= 1 && C >= 4 && (long long)B * H * W * C < (1LL << 38), "lpips_probe_relu_pool: bad shape");
    hipStream_t st = (hipStream_t)stream;
    return probe_finish(run_relu_pool(x_dev, y_dev, p_dev, (int)B, H, W, C, st), st);
}

int wmar_lpips_probe_relu_pool_backward(const float* y_dev, const float* gp_dev, const float* gt_dev, int64_t B, int32_t H, int32_t W, int32_t C,
                                        float* gx_dev, void* stream) {
    WMAR_REQUIRE(y_dev && gx_dev && (gp_dev || gt_dev), "lpips_probe_relu_pool_backward: null argument");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && H >= 1 && W >= 1 && C >= 4 && (long long)B * H * W * C < (1LL << 38),
                 "lpips_probe_relu_pool_backward: bad shape");
    hipStream_t st = (hipStream_t)stream;
    return probe_finish(run_relu_pool_backward(y_dev, gp_dev, gt_dev, gx_dev, (int)B, H, W, C, st), st);
}

int wmar_lpips_probe_head(const float* f0_dev, const float* f1_dev, const float* w_dev, int64_t B, int32_t HW, int32_t C, float* value_dev,
                          void* stream) {
    WMAR_REQUIRE(f0_dev && f1_dev && w_dev && value_dev, "lpips_probe_head: null argument");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && HW >= 1 && C >= 4, "lpips_probe_head: bad shape");
    hipStream_t st = (hipStream_t)stream;
    DeviceArena mem;
    int rc = WMAR_OK;
    float* n1 = nullptr;
    double* part = nullptr;
    WMAR_TRY(mem.alloc(&n1, (size_t)B * HW * C));
    WMAR_TRY(mem.alloc(&part, lpips_head_doubles((int)B, HW)));
    WMAR_TRY(run_lpips_normalize(f1_dev, n1, (int)B, HW, C, st));
    WMAR_TRY(run_lpips_head(f0_dev, n1, w_dev, part, value_dev, (int)B, HW, C, st));
    return probe_finish(rc, st);
}

int wmar_lpips_probe_head_backward(const float* f0_dev, const float* f1_dev, const float* w_dev, const float* grad_value_dev, int64_t B, int32_t HW,
                                   int32_t C, float* g0_dev, void* stream) {
    WMAR_REQUIRE(f0_dev && f1_dev && w_dev && grad_value_dev && g0_dev, "lpips_probe_head_backward: null argument");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && HW >= 1 && C >= 4, "lpips_probe_head_backward: bad shape");
    hipStream_t st = (hipStream_t)stream;
    DeviceArena mem;
    int rc = WMAR_OK;
    float* n1 = nullptr;
    WMAR_TRY(mem.alloc(&n1, (size_t)B * HW * C));
    WMAR_TRY(run_lpips_normalize(f1_dev, n1, (int)B, HW, C, st));
    WMAR_TRY(run_lpips_head_backward(f0_dev, n1, w_dev, grad_value_dev, g0_dev, (int)B, HW, C, st));
    return probe_finish(rc, st);
}

}  // extern "C"
