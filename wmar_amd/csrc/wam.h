// The WAM embedder (deps/watermark_anything: models/embedder.py VAEEmbedder, modules/vae.py VAEEncoder / VAEDecoder,
// modules/msg_processor.py "binary+concat", modules/jnd.py JND, models/wam.py Wam.blend / Wam.embed) and the reference's
// WamSync.add_sync (wmar/watermarking/synchronization.py:299-316) on the device.  Included by vqgan.hip: the network is a VqNet with
// plan_wam (vq_plan.h), loaded by net_load and executed by vq_forward; what this file adds is the three kernels around it
// (k_wam_latent_msg, k_wam_jnd, k_wam_tail), the NCHW -> NHWC input kernel and the engine that walks images and decoder rows.
//
// Pass structure of one call on B images with K messages per image (embed: K = 1, one message per image): the images are walked
// in groups of at most max_batch; per group ONE encoder pass (the latents do not depend on the message), one heat map launch, then the
// K * g decoder rows (row = image * K + message) in chunks of max_batch: k_wam_latent_msg, the decoder half, k_wam_tail.  Every output
// pixel is written by exactly one thread of one launch; there are no atomics, so two runs give the same bits.
#pragma once

namespace wmar {

// ImageNet colour constants in fp32, and the two the reference's unnormalize_img = Normalize(-mean / std, 1 / std) derives from them
struct WamColor { float mean[3], sd[3], umean[3], usd[3]; };

inline WamColor wam_color() {
    WamColor k;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    for (int c = 0; c < 3; ++c) { k.mean[c] = mean[c]; k.sd[c] = sd[c]; k.umean[c] = -mean[c] / sd[c]; k.usd[c] = 1.0f / sd[c]; }
    return k;
}

// how the images of a call arrive: in [0, 1], WAM-normalised, or in [-1, 1]
enum { WAM_IN_U01 = 0, WAM_IN_NORM = 1, WAM_IN_PM1 = 2 };

// the value the network sees (WamSync.normalize for images in [-1, 1])
__device__ __forceinline__ float wam_norm_in(float x, int mode, const WamColor& k, int c) {
#pragma clang fp contract(off)
    if (mode == WAM_IN_PM1) return ((x + 1.0f) / 2.0f - k.mean[c]) / k.sd[c];
    return x;
}
__device__ __forceinline__ float wam_unnorm(float xn, const WamColor& k, int c) {      // unnormalize_img
#pragma clang fp contract(off)
    return (xn - k.umean[c]) / k.usd[c];
}
__device__ __forceinline__ float wam_renorm(float u, const WamColor& k, int c) {       // normalize_img
#pragma clang fp contract(off)
    return (u - k.mean[c]) / k.sd[c];
}
__device__ __forceinline__ float f4_get(const float4& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }

// NCHW [B][3][HW] -> the encoder's input, NHWC [B][HW][8] (channels 3..7 zero), normalised.  Four pixels per thread.
__global__ __launch_bounds__(256) void k_wam_in(const float* __restrict__ src, float* __restrict__ dst, int HW, int mode, WamColor col) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long b = blockIdx.y;
    if (q * 4 >= HW) return;
    float4 ch[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) ch[c] = *(const float4*)(src + (b * 3 + c) * HW + q * 4);
    float* d = dst + (b * HW + q * 4) * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        *(float4*)(d + i * 8) = make_float4(wam_norm_in(f4_get(ch[0], i), mode, col, 0), wam_norm_in(f4_get(ch[1], i), mode, col, 1),
                                            wam_norm_in(f4_get(ch[2], i), mode, col, 2), 0.f);
        *(float4*)(d + i * 8 + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// The decoder's input (msg_processor.py:89-116, "binary+concat"): out [n][S2][Cs], NHWC, Cs = pad8(z + H), H = 2 * nbits.
// Row r = row0 + blockIdx.x takes channels 0..z-1 from the latents of image r / img_div (lat [images][S2][Ls], Ls = pad8(z)), the
// next H channels from sum_j table[2 j + bit_j] of message (msg_mod ? r % msg_mod : r), added in ascending j in fp32 once per row
// and broadcast over the pixels, and zeros in the padding channels.  A bit is "set" when it is not 0.
__global__ __launch_bounds__(256) void k_wam_latent_msg(const float* __restrict__ lat, const float* __restrict__ table,
                                                         const int* __restrict__ msgs, float* __restrict__ out, int S2, int z, int Ls,
                                                         int nbits, int Cs, int row0, int img_div, int msg_mod) {
    extern __shared__ __attribute__((aligned(16))) float rowv[];      // [Cs]
    const int H = 2 * nbits;
    const int r = row0 + blockIdx.x;
    const int img = r / img_div, msg = msg_mod ? r % msg_mod : r;
    for (int c = threadIdx.x; c < Cs; c += blockDim.x) {
        float s = 0.f;
        if (c >= z && c < z + H)
            for (int j = 0; j < nbits; ++j) s += table[(long long)(2 * j + (msgs[(long long)msg * nbits + j] != 0 ? 1 : 0)) * H + (c - z)];
        rowv[c] = s;
    }
    __syncthreads();
    const int q4 = Cs >> 2;
    const float* lb = lat + (long long)img * S2 * Ls;
    float* ob = out + (long long)blockIdx.x * S2 * Cs;
    for (int e = threadIdx.x; e < S2 * q4; e += blockDim.x) {
        const int pix = e / q4, c = (e - pix * q4) * 4;
        float4 v = *(const float4*)(rowv + c);
        if (c < z) {
            const float4 l = *(const float4*)(lb + (long long)pix * Ls + c);
            if (c + 0 < z) v.x = l.x;
            if (c + 1 < z) v.y = l.y;
            if (c + 2 < z) v.z = l.z;
            if (c + 3 < z) v.w = l.w;
        }
        *(float4*)(ob + (long long)pix * Cs + c) = v;
    }
}

// JND.heatmaps (jnd.py:65-110) for in_channels = 1: heat [B][R][R] = max(la + cm - 0.3 min(la, cm), 0) / 255 of the luminance
// 255 (0.299 r + 0.587 g + 0.114 b) of the image in [0, 1].  la: the 5 x 5 stencil / 32 through the two-branch curve; cm: the two
// 3 x 3 Sobel stencils, 0.117 * 16 g^2.4 / (g^2 + 26^2).  Zero padding of the LUMINANCE at the image border.  A 32 x 32 tile with a
// 2-pixel halo in LDS (staged as aligned groups of four pixels: columns x0 - 4 .. x0 + 35); four pixels per thread; the taps are added
// row by row, left to right.
constexpr int JND_T = 32, JND_LW = JND_T + 8, JND_LH = JND_T + 4;
__global__ __launch_bounds__(256) void k_wam_jnd(const float* __restrict__ src, float* __restrict__ heat, int R, int mode, WamColor col) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float lum[JND_LH][JND_LW];
    const long long b = blockIdx.z;
    const int x0 = blockIdx.x * JND_T, y0 = blockIdx.y * JND_T;
    const long long HW = (long long)R * R;
    const float* sb = src + b * 3 * HW;
    for (int e = threadIdx.x; e < JND_LH * (JND_LW / 4); e += 256) {
        const int ly = e / (JND_LW / 4), lq = e - ly * (JND_LW / 4);
        const int y = y0 - 2 + ly, x = x0 - 4 + lq * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (y >= 0 && y < R && x >= 0 && x < R) {      // R % 4 == 0: a group of four is inside or outside as a whole
            float o[4];
            const float4 r4 = *(const float4*)(sb + (long long)y * R + x), g4 = *(const float4*)(sb + HW + (long long)y * R + x),
                         b4 = *(const float4*)(sb + 2 * HW + (long long)y * R + x);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float rr = f4_get(r4, i), gg = f4_get(g4, i), bb = f4_get(b4, i);
                if (mode != WAM_IN_U01) {
                    rr = wam_unnorm(wam_norm_in(rr, mode, col, 0), col, 0);
                    gg = wam_unnorm(wam_norm_in(gg, mode, col, 1), col, 1);
                    bb = wam_unnorm(wam_norm_in(bb, mode, col, 2), col, 2);
                }
                o[i] = 0.299f * (255.0f * rr) + 0.587f * (255.0f * gg) + 0.114f * (255.0f * bb);
            }
            v = make_float4(o[0], o[1], o[2], o[3]);
        }
        *(float4*)&lum[ly][lq * 4] = v;
    }
    __syncthreads();
    const int ty = threadIdx.x >> 3, tq = threadIdx.x & 7;
    const int y = y0 + ty, x = x0 + tq * 4;
    if (y >= R || x >= R) return;
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int cy = ty + 2, cx = tq * 4 + i + 4;      // centre in the tile
        float s = 0.f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int ring = (dy == -2 || dy == 2 || dx == -2 || dx == 2) ? 1 : ((dy == 0 && dx == 0) ? 0 : 2);
                if (ring == 1) s += lum[cy + dy][cx + dx];
                else if (ring == 2) s += 2.0f * lum[cy + dy][cx + dx];
            }
        float la = s / 32.0f;
        la = la <= 127.0f ? 17.0f * (1.0f - sqrtf(la / 127.0f + 1e-5f)) : 3.0f / 128.0f * (la - 127.0f) + 3.0f;
        const float a00 = lum[cy - 1][cx - 1], a01 = lum[cy - 1][cx], a02 = lum[cy - 1][cx + 1];
        const float a10 = lum[cy][cx - 1], a12 = lum[cy][cx + 1];
        const float a20 = lum[cy + 1][cx - 1], a21 = lum[cy + 1][cx], a22 = lum[cy + 1][cx + 1];
        const float gx = -a00 + a02 - 2.0f * a10 + 2.0f * a12 - a20 + a22;
        const float gy = a00 + 2.0f * a01 + a02 - a20 - 2.0f * a21 - a22;
        float g = sqrtf(gx * gx + gy * gy);
        const float cm = 0.117f * (16.0f * powf(g, 2.4f) / (g * g + 676.0f));
        o[i] = fmaxf(la + cm - 0.3f * fminf(la, cm), 0.0f) / 255.0f;
    }
    *(float4*)(heat + b * HW + (long long)y * R + x) = make_float4(o[0], o[1], o[2], o[3]);
}

// The tail of Wam.embed / WamSync.add_sync for the decoder rows row0 .. row0 + n - 1 (gridDim.y = n), four pixels per thread:
//   d = tanh(y);  w = scaling_i * x + scaling_w * d;  attenuation in [0, 1] space: a = u + heat_c (u_w - u), normalised again.
// masks == null (embed): row r belongs to image r; out[r] = w', preds[r] = d (nullable).
// masks != null (add_sync): row r is message r % K of image r / K; a pixel is written by the row of the LAST message whose mask is
// set there (multi * (1 - m) + w * m over the messages in order, for 0/1 masks), or by the row of message 0 with the image itself
// where no mask is set; unnormalised, * 2 - 1, clamped to [-1, 1].
struct WamTailArgs {
    const float* y;                // [n][HW][Cy]: the decoder output, NHWC
    const float* img;              // [images][3][HW]
    const float* heat;             // [images][HW], null without attenuation
    const unsigned char* masks;    // [K][HW] or null
    float* out;                    // [images or rows][3][HW]
    float* preds;                  // nullable [rows][3][HW]
    int HW, Cy, row0, K, in_mode, att;
    float sw, si;
    WamColor col;
};
__global__ __launch_bounds__(256) void k_wam_tail(WamTailArgs a) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q * 4 >= a.HW) return;
    const long long p0 = q * 4;
    const int r = a.row0 + blockIdx.y;
    int img = r, k = 0;
    bool own[4] = {true, true, true, true}, pass[4] = {false, false, false, false};
    if (a.masks) {
        img = r / a.K; k = r - img * a.K;
        int sel[4] = {-1, -1, -1, -1};
        for (int kk = 0; kk < a.K; ++kk) {
            const unsigned m = *(const unsigned*)(a.masks + (long long)kk * a.HW + p0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if ((m >> (8 * i)) & 0xffu) sel[i] = kk;
        }
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) { pass[i] = sel[i] < 0; own[i] = sel[i] == k || (k == 0 && pass[i]); any = any || own[i]; }
        if (!any) return;
    }
    const float* yb = a.y + ((long long)blockIdx.y * a.HW + p0) * a.Cy;
    float4 yv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) yv[i] = *(const float4*)(yb + (long long)i * a.Cy);
    float4 hv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.att) hv = *(const float4*)(a.heat + (long long)img * a.HW + p0);
    const long long orow = a.masks ? img : r;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float4 xv = *(const float4*)(a.img + ((long long)img * 3 + c) * a.HW + p0);
        const float hw = (a.att == 2 && c < 2) ? 0.5f : 1.0f;      // jnd_1_3_blue: (0.5, 0.5, 1.0)
        float o[4], d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float xn = wam_norm_in(f4_get(xv, i), a.in_mode, a.col, c);
            d[i] = tanhf(f4_get(yv[i], c));
            float w = a.si * xn + a.sw * d[i];
            if (a.att) {
                const float u = wam_unnorm(xn, a.col, c), uw = wam_unnorm(w, a.col, c);
                w = wam_renorm(u + f4_get(hv, i) * hw * (uw - u), a.col, c);
            }
            if (a.masks) {
                const float v = wam_unnorm(pass[i] ? xn : w, a.col, c) * 2.0f - 1.0f;
                o[i] = fminf(fmaxf(v, -1.0f), 1.0f);
            } else {
                o[i] = w;
            }
        }
        float* op = a.out + (orow * 3 + c) * a.HW + p0;
        if (own[0] && own[1] && own[2] && own[3]) {
            *(float4*)op = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (own[i]) op[i] = o[i];
        }
        if (a.preds) *(float4*)(a.preds + ((long long)r * 3 + c) * a.HW + p0) = make_float4(d[0], d[1], d[2], d[3]);
    }
}

}  // namespace wmar

// ------------------------------------------------------------------------------ launches
namespace {

int run_wam_in(const float* src, float* dst, int B, int HW, int mode, const WamColor& col, hipStream_t st) {
    hipLaunchKernelGGL(k_wam_in, dim3((unsigned)((HW / 4 + 255) / 256), (unsigned)B), dim3(256), 0, st, src, dst, HW, mode, col);
    return launch_status("k_wam_in");
}

int run_wam_latent_msg(const float* lat, const float* table, const int* msgs, float* out, int n, int S2, int z, int nbits, int row0,
                       int img_div, int msg_mod, hipStream_t st) {
    const int Cs = pad8(z + 2 * nbits);
    hipLaunchKernelGGL(k_wam_latent_msg, dim3((unsigned)n), dim3(256), (size_t)Cs * sizeof(float), st, lat, table, msgs, out, S2, z, pad8(z),
                       nbits, Cs, row0, img_div, msg_mod);
    return launch_status("k_wam_latent_msg");
}

int run_wam_jnd(const float* src, float* heat, int B, int R, int mode, const WamColor& col, hipStream_t st) {
    const unsigned t = (unsigned)((R + JND_T - 1) / JND_T);
    hipLaunchKernelGGL(k_wam_jnd, dim3(t, t, (unsigned)B), dim3(256), 0, st, src, heat, R, mode, col);
    return launch_status("k_wam_jnd");
}

int run_wam_tail(const WamTailArgs& a, int n, hipStream_t st) {
    hipLaunchKernelGGL(k_wam_tail, dim3((unsigned)((a.HW / 4 + 255) / 256), (unsigned)n), dim3(256), 0, st, a);
    return launch_status("k_wam_tail");
}

bool wam_config_ok_for_tail(int R, int K, int att) { return R >= 4 && R % 4 == 0 && K >= 0 && K <= 8 && att >= 0 && att <= 2; }

}  // namespace

struct wmar_wam {
    DeviceArena mem;
    VqNet net;
    wmar_wam_config cfg{};
    WamColor col{};
    float* table = nullptr;      // msg_processor.msg_embeddings.weight [2 nbits][2 nbits]
    float* lat = nullptr;        // the encoder output of one image group [max_batch][S * S][pad8(z)]
    float* heat = nullptr;       // its heat maps [max_batch][R * R]
};

namespace {

// images [B][3][R][R] (in_mode) -> K messages each (masks != null: add_sync) or one message each (embed)
int wam_run(wmar_wam* w, const float* imgs, int64_t B, int in_mode, const int* msgs, int K, const unsigned char* masks, float* out,
            float* preds, hipStream_t st) {
    VqNet& n = w->net;
    const VqPlan& p = n.plan;
    const wmar_wam_config& c = w->cfg;
    const int R = p.resolution, HW = R * R, S2 = p.S * p.S, G = p.max_batch;
    const VqHalf &enc = p.half[0], &dec = p.half[1];
    int rc;
    for (int64_t g0 = 0; g0 < B; g0 += G) {
        const int g = (int)(B - g0 < G ? B - g0 : G);
        const float* gi = imgs + g0 * 3 * HW;
        if ((rc = run_wam_in(gi, n.at[enc.first], g, HW, in_mode, w->col, st))) return rc;
        if ((rc = vq_forward(n, enc, g, st))) return rc;
        // the decoder reuses the rotating buffers: the latents move out of them
        WMAR_HIP_CHECK(hipMemcpyAsync(w->lat, n.at[enc.last], (size_t)g * S2 * p.t[enc.last].C * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (c.attenuation && (rc = run_wam_jnd(gi, w->heat, g, R, in_mode, w->col, st))) return rc;
        const int rows = g * K;
        for (int r0 = 0; r0 < rows; r0 += G) {
            const int nr = rows - r0 < G ? rows - r0 : G;
            if ((rc = run_wam_latent_msg(w->lat, w->table, masks ? msgs : msgs + g0 * c.nbits, n.at[dec.first], nr, S2, c.z_channels, c.nbits, r0,
                                         K, masks ? K : 0, st))) return rc;
            if ((rc = vq_forward(n, dec, nr, st))) return rc;
            WamTailArgs a{};
            a.y = n.at[dec.last]; a.img = gi; a.heat = c.attenuation ? w->heat : nullptr; a.masks = masks;
            a.out = out + g0 * 3 * HW; a.preds = preds ? preds + g0 * 3 * HW : nullptr;
            a.HW = HW; a.Cy = p.t[dec.last].C; a.row0 = r0; a.K = K; a.in_mode = in_mode; a.att = c.attenuation;
            a.sw = c.scaling_w; a.si = c.scaling_i; a.col = w->col;
            if ((rc = run_wam_tail(a, nr, st))) return rc;
        }
    }
    return WMAR_OK;
}

}  // namespace

extern "C" {

int wmar_wam_create(const wmar_wam_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream,
                    wmar_wam** out) {
    WMAR_REQUIRE(cfg && names && tensors_dev && out, "wam_create: null argument");
    WMAR_REQUIRE(cfg->attenuation >= 0 && cfg->attenuation <= 2, "wam_create: attenuation %d (0 none, 1 jnd_1_3, 2 jnd_1_3_blue)", cfg->attenuation);
    VqPlan plan = plan_wam(*cfg, "wam_create");
    WMAR_REQUIRE(plan.err.empty(), "%s", plan.err.c_str());
    std::unique_ptr<wmar_wam> v(new wmar_wam());
    v->cfg = *cfg; v->col = wam_color();
    VqNet& n = v->net;
    n.plan = std::move(plan);
    const VqPlan& p = n.plan;
    hipStream_t st = (hipStream_t)stream;
    Loader ld(names, tensors_dev, n_tensors, &v->mem, st);
    int& rc = ld.rc;
    net_load(n, ld);
    const size_t H = (size_t)2 * cfg->nbits;
    const float* table = ld.need("msg_processor.msg_embeddings.weight");
    WMAR_TRY(v->mem.alloc(&v->table, H * H));
    if (rc == WMAR_OK && hipMemcpyAsync(v->table, table, H * H * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        set_error("wam_create: message table copy failed"); rc = WMAR_EHIP;
    }
    // ---- one buffer per slot, as large as the largest tensor the plan puts there (as the tokenizer engines)
    const size_t B = (size_t)p.max_batch;
    float* slot[VQ_SLOTS] = {};
    for (int s = 0; s < VQ_SLOTS; ++s)
        if (s < 4 || p.att_elems) WMAR_TRY(v->mem.alloc(&slot[s], B * (s < 4 ? p.rot_elems : p.att_elems)));
    for (const VqTensor& t : p.t) n.at.push_back(slot[t.slot]);
    if (p.attn_nn) WMAR_TRY(v->mem.alloc(&n.att.asc, B * p.attn_nn));
    net_scratch(n, v->mem, rc, st);
    WMAR_TRY(v->mem.alloc(&v->lat, B * p.S * p.S * pad8(cfg->z_channels)));
    WMAR_TRY(v->mem.alloc(&v->heat, B * p.resolution * p.resolution));
    if (rc == WMAR_OK && hipStreamSynchronize(st) != hipSuccess) { set_error("wam_create: sync failed"); rc = WMAR_EHIP; }
    if (rc != WMAR_OK) return rc;
    *out = v.release();
    return WMAR_OK;
}
void wmar_wam_destroy(wmar_wam* w) { delete w; }
int64_t wmar_wam_device_bytes(const wmar_wam* w) { return w ? w->mem.bytes : 0; }

int wmar_wam_embed(wmar_wam* w, const float* imgs_norm_dev, int64_t B, int32_t R, const int32_t* msgs_dev, float* imgs_w_dev,
                   float* preds_w_dev, void* stream) {
    WMAR_REQUIRE(w && imgs_norm_dev && msgs_dev && imgs_w_dev, "wam_embed: null argument");
    WMAR_REQUIRE(B >= 1, "wam_embed: batch %lld", (long long)B);
    WMAR_REQUIRE(R == w->cfg.resolution, "wam_embed: images of %d x %d, the embedder works at %d x %d", R, R, w->cfg.resolution, w->cfg.resolution);
    return wam_run(w, imgs_norm_dev, B, WAM_IN_NORM, msgs_dev, 1, nullptr, imgs_w_dev, preds_w_dev, (hipStream_t)stream);
}

int wmar_wam_add_sync(wmar_wam* w, const float* imgs_pm1_dev, int64_t B, int32_t R, const int32_t* msgs_dev, int32_t K,
                      const uint8_t* masks_dev, float* out_pm1_dev, void* stream) {
    WMAR_REQUIRE(w && imgs_pm1_dev && msgs_dev && masks_dev && out_pm1_dev, "wam_add_sync: null argument");
    WMAR_REQUIRE(B >= 1, "wam_add_sync: batch %lld", (long long)B);
    WMAR_REQUIRE(K >= 1 && K <= 8, "wam_add_sync: %d messages outside 1..8", K);
    WMAR_REQUIRE(R == w->cfg.resolution, "wam_add_sync: images of %d x %d, the embedder works at %d x %d", R, R, w->cfg.resolution,
                 w->cfg.resolution);
    return wam_run(w, imgs_pm1_dev, B, WAM_IN_PM1, msgs_dev, K, masks_dev, out_pm1_dev, nullptr, (hipStream_t)stream);
}

// ---- probes (tests, debugging): one kernel at a time; none is used by an engine path; each waits for the stream
int wmar_wam_probe_jnd(const float* imgs01_dev, int64_t B, int32_t R, float* heat_dev, void* stream) {
    WMAR_REQUIRE(imgs01_dev && heat_dev, "wam_probe_jnd: null argument");
    WMAR_REQUIRE(B >= 1 && B <= 65535 && R >= 4 && R % 4 == 0, "wam_probe_jnd: batch %lld (1..65535), size %d (a multiple of 4)", (long long)B, R);
    hipStream_t st = (hipStream_t)stream;
    return probe_finish(run_wam_jnd(imgs01_dev, heat_dev, (int)B, R, WAM_IN_U01, wam_color(), st), st);
}

int wmar_wam_probe_latent_msg(const float* latents_dev, int64_t n_images, int32_t S, int32_t z_channels, int32_t nbits,
                              const float* table_dev, const int32_t* msgs_dev, int64_t n_msgs, int64_t rows, int32_t img_div,
                              int32_t msg_mod, float* out_dev, void* stream) {
    WMAR_REQUIRE(latents_dev && table_dev && msgs_dev && out_dev, "wam_probe_latent_msg: null argument");
    WMAR_REQUIRE(S >= 1 && z_channels >= 1 && nbits >= 1 && nbits <= 64, "wam_probe_latent_msg: S %d, z_channels %d, nbits %d (1..64)", S,
                 z_channels, nbits);
    WMAR_REQUIRE(rows >= 1 && rows <= 65535 && img_div >= 1 && msg_mod >= 0, "wam_probe_latent_msg: rows %lld, img_div %d, msg_mod %d",
                 (long long)rows, img_div, msg_mod);
    WMAR_REQUIRE((rows - 1) / img_div < n_images && (msg_mod ? msg_mod : rows) <= n_msgs,
                 "wam_probe_latent_msg: %lld rows need %lld images and %lld messages, got %lld and %lld", (long long)rows,
                 (long long)((rows - 1) / img_div + 1), (long long)(msg_mod ? msg_mod : rows), (long long)n_images, (long long)n_msgs);
    hipStream_t st = (hipStream_t)stream;
    return probe_finish(run_wam_latent_msg(latents_dev, table_dev, msgs_dev, out_dev, (int)rows, S * S, z_channels, nbits, 0, img_div, msg_mod, st), st);
}

int wmar_wam_probe_tail(const float* y_dev, const float* imgs_dev, int32_t in_mode, int64_t B, int32_t R, const uint8_t* masks_dev,
                        int32_t K, float scaling_w, float scaling_i, int32_t attenuation, float* out_dev, float* preds_dev, void* stream) {
    WMAR_REQUIRE(y_dev && imgs_dev && out_dev, "wam_probe_tail: null argument");
    WMAR_REQUIRE(B >= 1 && wam_config_ok_for_tail(R, K, attenuation) && (masks_dev ? K >= 1 : true) && (in_mode == WAM_IN_NORM || in_mode == WAM_IN_PM1),
                 "wam_probe_tail: batch %lld, size %d, K %d (1..8 with masks), attenuation %d (0..2), in_mode %d (1 normalised, 2 [-1, 1])",
                 (long long)B, R, K, attenuation, in_mode);
    const int64_t rows = masks_dev ? B * K : B;
    WMAR_REQUIRE(B <= 65535 && rows <= 65535, "wam_probe_tail: %lld rows (at most 65535)", (long long)rows);
    hipStream_t st = (hipStream_t)stream;
    DeviceArena mem;
    float* heat = nullptr;
    int rc = WMAR_OK;
    const WamColor col = wam_color();
    if (attenuation) {
        WMAR_TRY(mem.alloc(&heat, (size_t)B * R * R));
        WMAR_TRY(run_wam_jnd(imgs_dev, heat, (int)B, R, in_mode, col, st));
    }
    if (rc == WMAR_OK) {
        WamTailArgs a{};
        a.y = y_dev; a.img = imgs_dev; a.heat = heat; a.masks = masks_dev; a.out = out_dev; a.preds = masks_dev ? nullptr : preds_dev;
        a.HW = R * R; a.Cy = 8; a.row0 = 0; a.K = masks_dev ? K : 1; a.in_mode = in_mode; a.att = attenuation; a.sw = scaling_w; a.si = scaling_i;
        a.col = col;
        rc = run_wam_tail(a, (int)rows, st);
    }
    return probe_finish(rc, st);
}

}  // extern "C"
