// The WAM extractor (deps/watermark_anything: models/extractor.py SegmentationExtractor = modules/vit.py ImageEncoderViT +
// modules/pixel_decoder.py PixelDecoder; models/wam.py Wam.detect without the resize) on the device: preds [B][nbits + 1][R][R] =
// pixel_decoder(image_encoder(x)) for images of the network's own size.  Included by vqgan.hip behind wam.h.
//
// Activations are NHWC fp32 with channels padded to a multiple of 8 (padding channels are zero), tokens are the pixels of a
// grid x grid image, so every Linear is a 1 x 1 convolution.  What this file adds to the conv path of vqgan.hip:
//   k_wx_conv      k_conv's implicit GEMM on the fp32-input MFMA (same weight packing, same 8 x 8 pixel tile, same accumulation
//                  order) with the staging modes the extractor needs -- per-token LayerNorm (+ GELU) applied while the patch is
//                  staged, the patch-embedding gather from the NCHW image, and bilinear upsampling + ReflectionPad2d(1) computed
//                  from the (at most four) source pixels of every patch pixel, so that neither a normalised nor an upsampled
//                  tensor ever exists in HBM -- and an epilogue with bias, residual (pos_embed: one image for the batch), exact
//                  GELU and an NCHW store for the last layer.
//   k_wx_ln_stats  (mean, rstd) per token over its channels, fp64 sums in a fixed order.
//   k_wx_attn      one launch per block: QK^T, the two decomposed rel-pos terms, softmax and PV of one (image, head, window) per
//                  workgroup, K and V of the window in LDS (sized by the window, not by the largest case).
// The Linears whose input needs nothing applied (attn.proj, mlp.lin2, neck.0) go through run_conv as they are (k_conv_bx).
// Pass structure per group of at most max_batch images: patch embedding; per block ln_stats, qkv, attention, proj (+ residual, in
// place), ln_stats, lin1 (+ GELU), lin2 (+ residual, in place); neck.0, ln_stats, neck.2, ln_stats; per stage the upsampling conv
// and ln_stats of its output; the last layer.  Every output element is written by exactly one thread of one launch and every sum
// runs in a fixed order: two runs give the same bits, and no value crosses a group.
#pragma once

namespace wmar {

// staging modes of k_wx_conv; WX_LN without a (mean, rstd) table stages the input as it is
enum { WX_LN = 1, WX_PATCH = 2, WX_UPS = 3 };

struct WxConvArgs {
    const float* in;          // NHWC [B][Hs][Ws][Cin];  WX_PATCH: the NCHW image [B][3][R][R]
    const float4* wp;         // k_pack_conv
    const float* bias;        // [CT * 32]
    const float* res;         // nullable NHWC [B or 1][Ho][Wo][Cout_s]
    long long res_bstride;    // floats between the residuals of two images (0: one for the batch)
    float* out;               // NHWC [B][Ho][Wo][Cout_s], or NCHW [B][Cout][Ho][Wo] (nchw)
    int Hs, Ws, Cin;          // Cin: stored input channels (the K of the GEMM), a multiple of 8
    int Ho, Wo, Cout_s, Cout;
    int CT, KBc, ks, pad;
    int tiles_x, tiles_y;
    // LayerNorm of the INPUT: (mean, rstd) per stored pixel, gamma / beta per channel (zero in the padding channels), then GELU
    const float2* ln_mr;
    const float* ln_g; const float* ln_b;
    int ln_gelu;
    int up_f;                 // WX_UPS: the conv sees the input upsampled by up_f (bilinear, align_corners = False), reflected by 1
    int patch, R;             // WX_PATCH: patch size and image size
    int gelu_out, nchw;
};

__device__ __forceinline__ float wx_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// four channels of one stored pixel as the conv sees them: LayerNorm (+ GELU) applied
__device__ __forceinline__ float4 wx_src(const WxConvArgs& a, const float* inb, long long tok0, int y, int x, int c) {
    const int p = y * a.Ws + x;
    float4 v = *(const float4*)(inb + (long long)p * a.Cin + c);
    if (a.ln_mr) {
        const float2 m = a.ln_mr[tok0 + p];
        const float4 g = *(const float4*)(a.ln_g + c), bt = *(const float4*)(a.ln_b + c);
        v = make_float4((v.x - m.x) * m.y * g.x + bt.x, (v.y - m.x) * m.y * g.y + bt.y, (v.z - m.x) * m.y * g.z + bt.z,
                        (v.w - m.x) * m.y * g.w + bt.w);
        if (a.ln_gelu) v = make_float4(wx_gelu(v.x), wx_gelu(v.y), wx_gelu(v.z), wx_gelu(v.w));
    }
    return v;
}

// bilinear source of upsampled coordinate d (nn.Upsample, align_corners = False): src = max(0, (d + 0.5) / f - 0.5), the upper
// neighbour clamped, lambda1 = src - floor(src), lambda0 = 1 - lambda1 (f a power of two: 1 / f and the products are exact)
__device__ __forceinline__ void wx_tap(int d, int f, int n, int& i0, int& i1, float& l0, float& l1) {
    const float s = fmaxf(((float)d + 0.5f) * (1.0f / (float)f) - 0.5f, 0.0f);
    i0 = (int)s;
    i1 = min(i0 + 1, n - 1);
    l1 = s - (float)i0;
    l0 = 1.0f - l1;
}

// four channels (c .. c + 3 of the GEMM's K) of patch pixel (y, x) in the coordinates the conv sees
template <int MODE>
__device__ __forceinline__ float4 wx_stage(const WxConvArgs& a, int b, int y, int x, int c) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MODE == WX_PATCH) {
        // K index c = (channel, dy, dx) of the patch of token (y, x): four consecutive dx are one aligned float4 of the image row
        const int pp = a.patch * a.patch;
        const int ch = c / pp, r = c - ch * pp, dy = r / a.patch, dx = r - dy * a.patch;
        if (ch >= 3) return zero;
        return *(const float4*)(a.in + (((long long)b * 3 + ch) * a.R + (long long)y * a.patch + dy) * a.R + (long long)x * a.patch + dx);
    }
    const float* inb = a.in + (long long)b * a.Hs * a.Ws * a.Cin;
    const long long tok0 = (long long)b * a.Hs * a.Ws;
    if (MODE == WX_UPS) {
        // ReflectionPad2d(1) of the UPSAMPLED tensor first: row -1 is row 1, row Ho is row Ho - 2
        y = y < 0 ? -y : (y >= a.Ho ? 2 * a.Ho - 2 - y : y);
        x = x < 0 ? -x : (x >= a.Wo ? 2 * a.Wo - 2 - x : x);
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        wx_tap(y, a.up_f, a.Hs, y0, y1, ly0, ly1);
        wx_tap(x, a.up_f, a.Ws, x0, x1, lx0, lx1);
        const float4 v00 = wx_src(a, inb, tok0, y0, x0, c), v01 = wx_src(a, inb, tok0, y0, x1, c);
        const float4 v10 = wx_src(a, inb, tok0, y1, x0, c), v11 = wx_src(a, inb, tok0, y1, x1, c);
        return make_float4(ly0 * (lx0 * v00.x + lx1 * v01.x) + ly1 * (lx0 * v10.x + lx1 * v11.x),
                           ly0 * (lx0 * v00.y + lx1 * v01.y) + ly1 * (lx0 * v10.y + lx1 * v11.y),
                           ly0 * (lx0 * v00.z + lx1 * v01.z) + ly1 * (lx0 * v10.z + lx1 * v11.z),
                           ly0 * (lx0 * v00.w + lx1 * v01.w) + ly1 * (lx0 * v10.w + lx1 * v11.w));
    }
    if (y < 0 || y >= a.Hs || x < 0 || x >= a.Ws) return zero;      // zero padding of the NORMALISED tensor (neck.2)
    return wx_src(a, inb, tok0, y, x, c);
}

// Epilogue: bias (+ residual) (+ GELU), NHWC store -- or the first Cout channels as NCHW.  Lane layout as conv_store.
__device__ __forceinline__ void wx_store(const WxConvArgs& a, const f32x16 (&acc)[2], int b, int ct, int ty, int tx, int lane) {
    const int j = lane & 31, half = lane >> 5;
    const int prow = j >> 3, pcol = j & 7;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int oy = ty * 8 + p * 4 + prow, ox = tx * 8 + pcol;
        const long long pin = (long long)oy * a.Wo + ox;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = ct * 32 + g * 8 + half * 4;
            if (co >= a.Cout_s) continue;
            const float4 bb = *(const float4*)(a.bias + co);
            float o[4] = {acc[p][g * 4 + 0] + bb.x, acc[p][g * 4 + 1] + bb.y, acc[p][g * 4 + 2] + bb.z, acc[p][g * 4 + 3] + bb.w};
            if (a.res) {
                const float4 rr = *(const float4*)(a.res + (long long)b * a.res_bstride + pin * a.Cout_s + co);
                o[0] += rr.x; o[1] += rr.y; o[2] += rr.z; o[3] += rr.w;
            }
            if (a.gelu_out)
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = wx_gelu(o[i]);
            if (a.nchw) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (co + i < a.Cout) a.out[((long long)b * a.Cout + co + i) * a.Ho * a.Wo + pin] = o[i];
            } else {
                *(float4*)(a.out + ((long long)b * a.Ho * a.Wo + pin) * a.Cout_s + co) = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
    }
}

// k_conv (stride 1) with the staging modes above: a workgroup owns an 8 x 8 output tile and COT cout tiles (one per wave); the
// patch of 32 input channels at a time goes through LDS.
template <int COT, int MODE>
__global__ __launch_bounds__(COT * 64) void k_wx_conv(WxConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float patch[];  // [PW * PW][CONV_PSTRIDE]
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int bid = blockIdx.x;
    const int tx = bid % a.tiles_x; bid /= a.tiles_x;
    const int ty = bid % a.tiles_y; bid /= a.tiles_y;
    const int cgroups = (a.CT + COT - 1) / COT;
    const int cg = bid % cgroups;
    const int b = bid / cgroups;
    const int ct = cg * COT + w;
    const bool active = ct < a.CT;
    const int T = a.ks * a.ks;
    const int PW = 7 + a.ks;
    const int iy0 = ty * 8 - a.pad, ix0 = tx * 8 - a.pad;

    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const int j = lane & 31, half = lane >> 5;
    const int prow = j >> 3, pcol = j & 7;

    for (int c0 = 0; c0 < a.Cin; c0 += CONV_CCH) {
        const int cch = min(CONV_CCH, a.Cin - c0);   // multiple of 8
        const int q4 = cch >> 2;                     // float4s per pixel this round
        __syncthreads();                             // the previous round's reads are done
        for (int e = threadIdx.x; e < PW * PW * q4; e += COT * 64) {
            const int pix = e / q4, qq = e - pix * q4;
            const int py = pix / PW, px = pix - py * PW;
            *(float4*)(patch + pix * CONV_PSTRIDE + qq * 4) = wx_stage<MODE>(a, b, iy0 + py, ix0 + px, c0 + qq * 4);
        }
        __syncthreads();
        if (active) {
            const int nkb = cch >> 3;
            const float4* wbase = a.wp + ((long long)ct * T * a.KBc + (c0 >> 3)) * 64 + lane;
            for (int tap = 0; tap < T; ++tap) {
                const int dy = tap / a.ks, dx = tap - dy * a.ks;
                const float4* wt = wbase + (long long)tap * a.KBc * 64;
                const float* p0 = patch + ((prow + dy) * PW + pcol + dx) * CONV_PSTRIDE + half * 4;
                const float* p1 = p0 + 4 * PW * CONV_PSTRIDE;
#pragma unroll 4
                for (int kb = 0; kb < nkb; ++kb) {
                    const float4 wv = wt[kb * 64];
                    const float4 x0 = *(const float4*)(p0 + kb * 8);
                    const float4 x1 = *(const float4*)(p1 + kb * 8);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.x, x0.x, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.x, x1.x, acc[1], 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.y, x0.y, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.y, x1.y, acc[1], 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.z, x0.z, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.z, x1.z, acc[1], 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.w, x0.w, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv.w, x1.w, acc[1], 0, 0, 0);
                }
            }
        }
    }
    if (!active) return;
    wx_store(a, acc, b, ct, ty, tx, lane);
}

// (mean, rstd) of every token over its C real channels (x [n][Cs], padding channels zero: they add nothing to either sum).  One
// wave per token: per-lane fp64 sums over its float4s in ascending order, then a fixed butterfly over the lanes.
__global__ __launch_bounds__(256) void k_wx_ln_stats(const float* __restrict__ x, float2* __restrict__ mr, long long n, int C, int Cs, float eps) {
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= n) return;
    const float* xt = x + t * Cs;
    double s = 0.0, ss = 0.0;
    for (int c = lane * 4; c < Cs; c += 256) {
        const float4 v = *(const float4*)(xt + c);
        s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        ss += sq4_f64(v);      // never a v_fmac_f64 chain: common.h
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { s += __shfl_xor(s, o); ss += __shfl_xor(ss, o); }
    if (lane == 0) {
        const double rn = inv_count_f64((double)C);
        const double mean = s * rn;
        double var = var_f64(ss * rn, mean);
        var = var > 0.0 ? var : 0.0;
        mr[t] = make_float2((float)mean, (float)rsqrt_f64(var + (double)eps));
    }
}

// Attention of one block.  qkv NHWC [B][g][g][3 D], channel which * D + head * hd + c;  out [B][g][g][D], channel head * hd + c.
// blockIdx.x = (image, head, window): the window's S x S tokens (S = g: one window, a global block).  K (rows padded by 4 floats:
// the 16-byte reads of 16 consecutive rows fall on different banks) and V of the window in LDS; a wave takes every 4th query:
// lanes over keys for the scores (the dot product in ascending c, + rel_h[q, ky] + rel_w[q, kx] of the UNSCALED q), a butterfly
// for max and sum, lanes over channels for PV (ascending key).
struct WxAttnArgs {
    const float* qkv; float* out;
    const float* rel_h; const float* rel_w;      // [2 S - 1][hd]
    int g, S, nh, hd, D;
    float scale;
};

__global__ __launch_bounds__(256) void k_wx_attn(WxAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int S = a.S, N = S * S, hd = a.hd, KS = hd + 4;
    float* Ks = lds;                                  // [N][hd + 4]
    float* Vs = Ks + (size_t)N * KS;                  // [N][hd]
    const int per_wave = (2 * hd + N + 2 * S + 3) & ~3;          // keeps every wave's qs 16-byte aligned
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float* qs = Vs + (size_t)N * hd + (size_t)w * per_wave;      // [hd] scaled q
    float* qu = qs + hd;                                          // [hd] q
    float* sc = qu + hd;                                          // [N]
    float* rh = sc + N;                                           // [S]
    float* rw = rh + S;                                           // [S]
    const int nw = a.g / S;
    int bid = blockIdx.x;
    const int win = bid % (nw * nw); bid /= nw * nw;
    const int head = bid % a.nh;
    const int b = bid / a.nh;
    const int wy = win / nw, wx = win - wy * nw;
    const long long row = 3LL * a.D;
    const float* base = a.qkv + (long long)b * a.g * a.g * row + head * hd;
    const int q4 = hd >> 2;
    for (int e = threadIdx.x; e < N * q4; e += 256) {
        const int n = e / q4, c = (e - n * q4) * 4;
        const int iy = n / S, ix = n - iy * S;
        const float* tokp = base + ((long long)(wy * S + iy) * a.g + wx * S + ix) * row;
        *(float4*)(Ks + n * KS + c) = *(const float4*)(tokp + a.D + c);
        *(float4*)(Vs + n * hd + c) = *(const float4*)(tokp + 2 * a.D + c);
    }
    for (int i0 = 0; i0 < N; i0 += 4) {
        const int i = i0 + w;
        const bool on = i < N;
        const int qy = on ? i / S : 0, qx = on ? i - qy * S : 0;
        const long long tok = (long long)(wy * S + qy) * a.g + wx * S + qx;
        __syncthreads();                              // K / V staged; the previous query's reads of qs .. rw are done
        if (on && lane < hd) {
            const float v = base[tok * row + lane];
            qu[lane] = v;
            qs[lane] = v * a.scale;
        }
        __syncthreads();
        if (on && lane < 2 * S) {
            const int k = lane < S ? lane : lane - S;
            const float* tab = (lane < S ? a.rel_h + (long long)(qy - k + S - 1) * hd : a.rel_w + (long long)(qx - k + S - 1) * hd);
            float s = 0.f;
            for (int c = 0; c < hd; ++c) s += qu[c] * tab[c];
            (lane < S ? rh : rw)[k] = s;
        }
        __syncthreads();
        float mx = -INFINITY;
        if (on)
            for (int jk = lane; jk < N; jk += 64) {
                const float* kr = Ks + jk * KS;
                float s = 0.f;
                for (int c = 0; c < hd; c += 4) {
                    const float4 kv = *(const float4*)(kr + c), qv = *(const float4*)(qs + c);
                    s += qv.x * kv.x; s += qv.y * kv.y; s += qv.z * kv.z; s += qv.w * kv.w;
                }
                const int ky = jk / S, kx = jk - ky * S;
                s = (s + rh[ky]) + rw[kx];
                sc[jk] = s;
                mx = fmaxf(mx, s);
            }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        float sum = 0.f;
        if (on)
            for (int jk = lane; jk < N; jk += 64) {
                const float e = expf(sc[jk] - mx);
                sc[jk] = e;
                sum += e;
            }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
        if (on)
            for (int jk = lane; jk < N; jk += 64) sc[jk] = sc[jk] / sum;
        __syncthreads();
        if (on && lane < hd) {
            float o = 0.f;
            for (int jk = 0; jk < N; ++jk) o += sc[jk] * Vs[jk * hd + lane];
            a.out[((long long)b * a.g * a.g + tok) * a.D + head * hd + lane] = o;
        }
    }
}

}  // namespace wmar

// ------------------------------------------------------------------------------ launches
namespace {

// LDS of one k_wx_attn workgroup
size_t wx_attn_lds(int S, int hd) { const size_t N = (size_t)S * S; return (N * (2 * hd + 4) + 4 * ((2 * hd + N + 2 * S + 3) & ~(size_t)3)) * sizeof(float); }
constexpr size_t WX_ATTN_LDS_MAX = 160 * 1024;
bool wx_attn_ok(int S, int hd) { return S >= 1 && S <= 32 && hd >= 4 && hd <= 64 && hd % 4 == 0 && wx_attn_lds(S, hd) <= WX_ATTN_LDS_MAX; }

// a normalisation applied by the consuming conv
struct WxLnRef { const float2* mr; const float* g; const float* b; int gelu; };

// c: the packed weights (Loader::conv);  in / out as WxConvArgs;  Hs: stored input size (WX_PATCH: the grid);  f: WX_UPS factor
int run_wx_conv(int mode, const ConvW& c, const float* in, float* out, int B, int Hs, int f, const WxLnRef* ln, const float* res,
                long long res_bstride, int gelu_out, int nchw, int patch, hipStream_t st) {
    WxConvArgs a{};
    a.in = in; a.wp = c.wp; a.bias = c.bias; a.res = res; a.res_bstride = res_bstride; a.out = out;
    a.Hs = a.Ws = Hs; a.Cin = c.cin_s;
    a.Ho = a.Wo = mode == WX_UPS ? Hs * f : Hs;
    a.Cout_s = c.cout_s; a.Cout = c.cout; a.CT = c.CT; a.KBc = c.KBc; a.ks = c.ks; a.pad = c.ks == 3 ? 1 : 0;
    a.up_f = f; a.patch = patch; a.R = Hs * patch; a.gelu_out = gelu_out; a.nchw = nchw;
    if (ln) { a.ln_mr = ln->mr; a.ln_g = ln->g; a.ln_b = ln->b; a.ln_gelu = ln->gelu; }
    WMAR_REQUIRE(a.Ho % 8 == 0, "wamx conv: output %d x %d is not a multiple of the 8 x 8 tile", a.Ho, a.Wo);
    WMAR_REQUIRE((c.ks == 1 || c.ks == 3) && (mode != WX_UPS || (c.ks == 3 && Hs >= 2)) && (mode != WX_PATCH || (c.ks == 1 && patch % 4 == 0)),
                 "wamx conv: kernel size %d in staging mode %d", c.ks, mode);
    a.tiles_x = a.Wo / 8; a.tiles_y = a.Ho / 8;
    const int PW = 7 + c.ks;
    const int COT = c.CT >= 4 ? 4 : (c.CT >= 2 ? 2 : 1);
    const size_t lds = (size_t)PW * PW * CONV_PSTRIDE * sizeof(float);
    const int cgroups = (c.CT + COT - 1) / COT;
    const long long grid = (long long)B * cgroups * a.tiles_x * a.tiles_y;
    WMAR_REQUIRE(grid >= 1 && grid < (1LL << 31), "wamx conv: grid of %lld workgroups", grid);
#define WMAR_WX_LAUNCH(MODE)                                                                                                   \
    if (COT == 4) hipLaunchKernelGGL((k_wx_conv<4, MODE>), dim3((unsigned)grid), dim3(256), lds, st, a);                        \
    else if (COT == 2) hipLaunchKernelGGL((k_wx_conv<2, MODE>), dim3((unsigned)grid), dim3(128), lds, st, a);                   \
    else hipLaunchKernelGGL((k_wx_conv<1, MODE>), dim3((unsigned)grid), dim3(64), lds, st, a);
    if (mode == WX_PATCH) { WMAR_WX_LAUNCH(WX_PATCH) }
    else if (mode == WX_UPS) { WMAR_WX_LAUNCH(WX_UPS) }
    else { WMAR_WX_LAUNCH(WX_LN) }       // without ln_mr the same staging is the plain one
#undef WMAR_WX_LAUNCH
    return launch_status("k_wx_conv");
}

int run_wx_ln_stats(const float* x, float2* mr, long long n, int C, float eps, hipStream_t st) {
    hipLaunchKernelGGL(k_wx_ln_stats, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, x, mr, n, C, pad8(C), eps);
    return launch_status("k_wx_ln_stats");
}

int run_wx_attn(const float* qkv, float* out, const float* rel_h, const float* rel_w, int B, int g, int S, int nh, int hd, hipStream_t st) {
    WMAR_REQUIRE(wx_attn_ok(S, hd) && g % S == 0, "wamx attention: window %d of a grid of %d, head width %d", S, g, hd);
    static const hipError_t lds_ok = hipFuncSetAttribute((const void*)k_wx_attn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)WX_ATTN_LDS_MAX);
    WMAR_REQUIRE(lds_ok == hipSuccess, "k_wx_attn: raising the dynamic LDS limit failed: %s", hipGetErrorString(lds_ok));
    WxAttnArgs a{};
    a.qkv = qkv; a.out = out; a.rel_h = rel_h; a.rel_w = rel_w; a.g = g; a.S = S; a.nh = nh; a.hd = hd; a.D = nh * hd;
    a.scale = 1.0f / sqrtf((float)hd);      // head_dim ** -0.5
    const long long grid = (long long)B * nh * (g / S) * (g / S);
    WMAR_REQUIRE(grid >= 1 && grid < (1LL << 31), "wamx attention: grid of %lld workgroups", grid);
    hipLaunchKernelGGL(k_wx_attn, dim3((unsigned)grid), dim3(256), wx_attn_lds(S, hd), st, a);
    return launch_status("k_wx_attn");
}

// run_conv for the Linears whose input needs nothing applied.  run_conv consults the thread's GroupNorm statistics tracker (g_trk: a
// VQGAN call on this thread may have left it armed, and at widths of 128, 256 or 512 the conv would then write per-tile sums into that
// engine's scratch); the extractor has no GroupNorm, so the tracker is set aside for the call and put back.
int wx_run_conv(const ConvW& c, const float* in, float* out, const float* res, int B, int G, hipStream_t st) {
    const GnTrack keep = g_trk;
    g_trk = GnTrack{};
    const int rc = run_conv(c, in, out, res, B, G, G, 1, 0, st);
    g_trk = keep;
    return rc;
}

struct WxNorm { float* g = nullptr; float* b = nullptr; int C = 0; };
struct WxBlock { WxNorm n1, n2; ConvW qkv, proj, lin1, lin2; float* rel_h = nullptr; float* rel_w = nullptr; int S = 0; };
struct WxStage { ConvW conv; WxNorm ln; int f = 1; };

// gamma / beta with zeros in the padding channels
void wx_load_norm(Loader& ld, const std::string& p, int C, WxNorm& n) {
    const float* g = ld.need(p + ".weight");
    const float* b = ld.need(p + ".bias");
    int& rc = ld.rc;
    if (rc) return;
    n.C = C;
    WMAR_TRY(ld.v->alloc_zero(&n.g, (size_t)pad8(C), ld.st));
    WMAR_TRY(ld.v->alloc_zero(&n.b, (size_t)pad8(C), ld.st));
    if (rc == WMAR_OK && (hipMemcpyAsync(n.g, g, (size_t)C * 4, hipMemcpyDeviceToDevice, ld.st) != hipSuccess ||
                          hipMemcpyAsync(n.b, b, (size_t)C * 4, hipMemcpyDeviceToDevice, ld.st) != hipSuccess)) {
        set_error("wamx_create: norm copy failed"); rc = WMAR_EHIP;
    }
}

void wx_load_copy(Loader& ld, const std::string& name, size_t n, float** dst) {
    const float* src = ld.need(name);
    int& rc = ld.rc;
    if (rc) return;
    WMAR_TRY(ld.v->alloc(dst, n));
    if (rc == WMAR_OK && hipMemcpyAsync(*dst, src, n * 4, hipMemcpyDeviceToDevice, ld.st) != hipSuccess) {
        set_error("wamx_create: copy of %s failed", name.c_str()); rc = WMAR_EHIP;
    }
}

}  // namespace

struct wmar_wamx {
    DeviceArena mem;
    wmar_wamx_config cfg{};
    int grid = 0, hd = 0;
    ConvW patch;
    float* pos = nullptr;                 // [grid][grid][D]
    std::vector<WxBlock> blk;
    ConvW neck0, neck2;
    WxNorm neck1, neck3;
    std::vector<WxStage> stage;
    ConvW last;
    // activations of one image group
    float *x = nullptr, *wide = nullptr, *att = nullptr, *n1 = nullptr, *n2 = nullptr;
    float* up[4] = {};
    float2* mr = nullptr;                 // (mean, rstd) per pixel of the largest normalised tensor
};

namespace {

bool wx_is_global(const wmar_wamx_config& c, int i) {
    for (int k = 0; k < c.n_global; ++k)
        if (c.global_attn_indexes[k] == i) return true;
    return false;
}

// one block on the g images in w->x, in place
int wx_block(wmar_wamx* w, int i, int g, hipStream_t st) {
    const WxBlock& b = w->blk[i];
    const int G = w->grid, D = w->cfg.embed_dim;
    const long long T = (long long)g * G * G;
    int rc;
    if ((rc = run_wx_ln_stats(w->x, w->mr, T, D, 1e-5f, st))) return rc;
    WxLnRef l1{w->mr, b.n1.g, b.n1.b, 0};
    if ((rc = run_wx_conv(WX_LN, b.qkv, w->x, w->wide, g, G, 1, &l1, nullptr, 0, 0, 0, 0, st))) return rc;
    if ((rc = run_wx_attn(w->wide, w->att, b.rel_h, b.rel_w, g, G, b.S, w->cfg.num_heads, w->hd, st))) return rc;
    if ((rc = wx_run_conv(b.proj, w->att, w->x, w->x, g, G, st))) return rc;       // + shortcut, in place (each element read and
    if ((rc = run_wx_ln_stats(w->x, w->mr, T, D, 1e-5f, st))) return rc;                 //   written by the same thread)
    WxLnRef l2{w->mr, b.n2.g, b.n2.b, 0};
    if ((rc = run_wx_conv(WX_LN, b.lin1, w->x, w->wide, g, G, 1, &l2, nullptr, 0, 1, 0, 0, st))) return rc;      // GELU in the epilogue
    return wx_run_conv(b.lin2, w->wide, w->x, w->x, g, G, st);
}

int wx_run(wmar_wamx* w, const float* imgs, int64_t B, float* preds, hipStream_t st) {
    const wmar_wamx_config& c = w->cfg;
    const int R = c.img_size, G = w->grid, MB = c.max_batch;
    int rc;
    for (int64_t g0 = 0; g0 < B; g0 += MB) {
        const int g = (int)(B - g0 < MB ? B - g0 : MB);
        if ((rc = run_wx_conv(WX_PATCH, w->patch, imgs + g0 * 3 * R * R, w->x, g, G, 1, nullptr, w->pos, 0, 0, 0, c.patch_size, st))) return rc;
        for (int i = 0; i < c.depth; ++i)
            if ((rc = wx_block(w, i, g, st))) return rc;
        const long long T = (long long)g * G * G;
        if ((rc = wx_run_conv(w->neck0, w->x, w->n1, nullptr, g, G, st))) return rc;
        if ((rc = run_wx_ln_stats(w->n1, w->mr, T, c.out_chans, 1e-6f, st))) return rc;
        WxLnRef l1{w->mr, w->neck1.g, w->neck1.b, 0};
        if ((rc = run_wx_conv(WX_LN, w->neck2, w->n1, w->n2, g, G, 1, &l1, nullptr, 0, 0, 0, 0, st))) return rc;
        if ((rc = run_wx_ln_stats(w->n2, w->mr, T, c.out_chans, 1e-6f, st))) return rc;
        const float* prev = w->n2;
        WxLnRef ln{w->mr, w->neck3.g, w->neck3.b, 0};
        int H = G;
        for (size_t j = 0; j < w->stage.size(); ++j) {
            const WxStage& s = w->stage[j];
            if ((rc = run_wx_conv(WX_UPS, s.conv, prev, w->up[j], g, H, s.f, &ln, nullptr, 0, 0, 0, 0, st))) return rc;
            H *= s.f;
            if ((rc = run_wx_ln_stats(w->up[j], w->mr, (long long)g * H * H, s.conv.cout, 1e-6f, st))) return rc;
            prev = w->up[j];
            ln = WxLnRef{w->mr, s.ln.g, s.ln.b, 1};
        }
        if ((rc = run_wx_conv(WX_LN, w->last, prev, preds + g0 * (c.nbits + 1) * R * R, g, H, 1, &ln, nullptr, 0, 0, 1, 0, st))) return rc;
    }
    return WMAR_OK;
}

}  // namespace

extern "C" {

int wmar_wamx_create(const wmar_wamx_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream,
                     wmar_wamx** out) {
    WMAR_REQUIRE(cfg && names && tensors_dev && out, "wamx_create: null argument");
    const wmar_wamx_config& c = *cfg;
    WMAR_REQUIRE(c.img_size >= 1 && c.patch_size >= 1 && c.embed_dim >= 1 && c.depth >= 1 && c.num_heads >= 1 && c.window_size >= 1 &&
                 c.out_chans >= 1 && c.max_batch >= 1, "wamx_create: sizes must be positive");
    WMAR_REQUIRE(c.n_global >= 0 && c.n_global <= 16, "wamx_create: %d global blocks (at most 16)", c.n_global);
    for (int k = 0; k < c.n_global; ++k)
        WMAR_REQUIRE(c.global_attn_indexes[k] >= 0 && c.global_attn_indexes[k] < c.depth, "wamx_create: global block %d of %d blocks",
                     c.global_attn_indexes[k], c.depth);
    WMAR_REQUIRE(c.nbits >= 1 && c.nbits <= 64, "wamx_create: nbits %d outside 1..64", c.nbits);
    WMAR_REQUIRE(c.img_size % c.patch_size == 0 && c.patch_size % 4 == 0, "wamx_create: image of %d in patches of %d (a multiple of 4 that divides it)",
                 c.img_size, c.patch_size);
    const int G = c.img_size / c.patch_size;
    WMAR_REQUIRE(G % c.window_size == 0, "wamx_create: grid %d is no multiple of window_size %d (the reference pads such grids with zero "
                 "tokens that take part as keys; this is not built)", G, c.window_size);
    WMAR_REQUIRE(G % 8 == 0, "wamx_create: grid %d (and with it every upscaled size) is not a multiple of the 8 x 8 conv tile", G);
    WMAR_REQUIRE(c.embed_dim % c.num_heads == 0, "wamx_create: embed_dim %d is not divisible by num_heads %d", c.embed_dim, c.num_heads);
    const int hd = c.embed_dim / c.num_heads;
    WMAR_REQUIRE(c.embed_dim % 8 == 0, "wamx_create: embed_dim %d is not a multiple of 8", c.embed_dim);
    WMAR_REQUIRE(wx_attn_ok(c.window_size, hd) && (c.n_global == 0 || wx_attn_ok(G, hd)),
                 "wamx_create: head width %d with windows of %d and a grid of %d: the attention kernel takes multiples of 4 up to 64, "
                 "windows up to 32 x 32 and K, V of a window within %zu bytes of LDS", hd, c.window_size, G, WX_ATTN_LDS_MAX);
    WMAR_REQUIRE(c.n_stages >= 1 && c.n_stages <= 4, "wamx_create: %d upscaling stages (1..4)", c.n_stages);
    int prod = 1;
    for (int j = 0; j < c.n_stages; ++j) {
        WMAR_REQUIRE(c.upscale_stages[j] == 2 || c.upscale_stages[j] == 4 || c.upscale_stages[j] == 8, "wamx_create: upscaling factor %d (2, 4 or 8)",
                     c.upscale_stages[j]);
        prod *= c.upscale_stages[j];
    }
    WMAR_REQUIRE(c.out_chans % prod == 0, "wamx_create: out_chans %d is not divisible by the product of the stages %d", c.out_chans, prod);
    WMAR_REQUIRE(prod == c.patch_size, "wamx_create: the stages upscale by %d, the patch size is %d", prod, c.patch_size);

    std::unique_ptr<wmar_wamx> v(new wmar_wamx());
    v->cfg = c; v->grid = G; v->hd = hd;
    hipStream_t st = (hipStream_t)stream;
    Loader ld(names, tensors_dev, n_tensors, &v->mem, st);
    int& rc = ld.rc;
    const int D = c.embed_dim, C = c.out_chans;
    const std::string e = "image_encoder.", pd = "pixel_decoder.";
    ld.conv(e + "patch_embed.proj", 3 * c.patch_size * c.patch_size, D, 1, v->patch);
    wx_load_copy(ld, e + "pos_embed", (size_t)G * G * D, &v->pos);
    v->blk.resize(c.depth);
    for (int i = 0; i < c.depth && rc == WMAR_OK; ++i) {
        WxBlock& b = v->blk[i];
        const std::string p = e + "blocks." + std::to_string(i) + ".";
        b.S = wx_is_global(c, i) ? G : c.window_size;
        wx_load_norm(ld, p + "norm1", D, b.n1);
        wx_load_copy(ld, p + "attn.rel_pos_h", (size_t)(2 * b.S - 1) * hd, &b.rel_h);
        wx_load_copy(ld, p + "attn.rel_pos_w", (size_t)(2 * b.S - 1) * hd, &b.rel_w);
        ld.conv(p + "attn.qkv", D, 3 * D, 1, b.qkv);
        ld.conv(p + "attn.proj", D, D, 1, b.proj);
        wx_load_norm(ld, p + "norm2", D, b.n2);
        ld.conv(p + "mlp.lin1", D, 4 * D, 1, b.lin1);
        ld.conv(p + "mlp.lin2", 4 * D, D, 1, b.lin2);
    }
    ld.conv(e + "neck.0", D, C, 1, v->neck0, false);
    wx_load_norm(ld, e + "neck.1", C, v->neck1);
    ld.conv(e + "neck.2", C, C, 3, v->neck2, false);
    wx_load_norm(ld, e + "neck.3", C, v->neck3);
    v->stage.resize(c.n_stages);
    int ch = C;
    for (int j = 0; j < c.n_stages && rc == WMAR_OK; ++j) {
        WxStage& s = v->stage[j];
        const std::string p = pd + "output_upscaling." + std::to_string(j) + ".upsample_block.";
        s.f = c.upscale_stages[j];
        ld.conv(p + "2", ch, ch / s.f, 3, s.conv, false);
        wx_load_norm(ld, p + "3", ch / s.f, s.ln);
        ch /= s.f;
    }
    ld.conv(pd + "last_layer", ch, c.nbits + 1, 1, v->last);
    // ---- activations of one image group
    const size_t MB = (size_t)c.max_batch, T = MB * G * G;
    WMAR_TRY(v->mem.alloc(&v->x, T * D));
    WMAR_TRY(v->mem.alloc(&v->wide, T * 4 * D));
    WMAR_TRY(v->mem.alloc(&v->att, T * D));
    WMAR_TRY(v->mem.alloc(&v->n1, T * pad8(C)));
    WMAR_TRY(v->mem.alloc(&v->n2, T * pad8(C)));
    size_t H = G;
    ch = C;
    for (int j = 0; j < c.n_stages; ++j) {
        H *= c.upscale_stages[j]; ch /= c.upscale_stages[j];
        WMAR_TRY(v->mem.alloc(&v->up[j], MB * H * H * pad8(ch)));
    }
    WMAR_TRY(v->mem.alloc(&v->mr, MB * H * H));
    if (rc == WMAR_OK && hipStreamSynchronize(st) != hipSuccess) { set_error("wamx_create: sync failed"); rc = WMAR_EHIP; }
    if (rc != WMAR_OK) return rc;
    *out = v.release();
    return WMAR_OK;
}
void wmar_wamx_destroy(wmar_wamx* w) { delete w; }
int64_t wmar_wamx_device_bytes(const wmar_wamx* w) { return w ? w->mem.bytes : 0; }

int wmar_wamx_detect(wmar_wamx* w, const float* imgs_norm_dev, int64_t B, int32_t R, float* preds_dev, void* stream) {
    WMAR_REQUIRE(w && imgs_norm_dev && preds_dev, "wamx_detect: null argument");
    WMAR_REQUIRE(B >= 1, "wamx_detect: batch %lld", (long long)B);
    WMAR_REQUIRE(R == w->cfg.img_size, "wamx_detect: images of %d x %d, the extractor works at %d x %d", R, R, w->cfg.img_size, w->cfg.img_size);
    return wx_run(w, imgs_norm_dev, B, preds_dev, (hipStream_t)stream);
}

// ---- probes (tests, debugging): one kernel at a time through the launches the engine uses; each waits for the stream
int wmar_wamx_probe_layernorm(const float* x_dev, int64_t n, int32_t C, float eps, float* mr_dev, void* stream) {
    WMAR_REQUIRE(x_dev && mr_dev, "wamx_probe_layernorm: null argument");
    WMAR_REQUIRE(n >= 1 && n < (1LL << 32) && C >= 1, "wamx_probe_layernorm: %lld tokens of %d channels", (long long)n, C);
    hipStream_t st = (hipStream_t)stream;
    return probe_finish(run_wx_ln_stats(x_dev, (float2*)mr_dev, n, C, eps, st), st);
}

int wmar_wamx_probe_patch_embed(const float* imgs_dev, int64_t B, int32_t R, int32_t patch, const float* w_dev, const float* bias_dev,
                                const float* pos_dev, int32_t D, float* out_dev, void* stream) {
    WMAR_REQUIRE(imgs_dev && w_dev && bias_dev && pos_dev && out_dev, "wamx_probe_patch_embed: null argument");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && patch >= 4 && patch % 4 == 0 && R % patch == 0 && (R / patch) % 8 == 0 && D >= 1 && D % 8 == 0,
                 "wamx_probe_patch_embed: batch %lld (1..1024), size %d in patches of %d (a multiple of 4; a grid that is a multiple of 8), width %d "
                 "(a multiple of 8)", (long long)B, R, patch, D);
    hipStream_t st = (hipStream_t)stream;
    DeviceArena mem;
    const char* names[2] = {"probe.weight", "probe.bias"};
    const void* tensors[2] = {w_dev, bias_dev};
    Loader ld(names, tensors, 2, &mem, st);
    ConvW c;
    ld.conv("probe", 3 * patch * patch, D, 1, c);
    int rc = ld.rc;
    WMAR_TRY(run_wx_conv(WX_PATCH, c, imgs_dev, out_dev, (int)B, R / patch, 1, nullptr, pos_dev, 0, 0, 0, patch, st));
    return probe_finish(rc, st);
}

int wmar_wamx_probe_attn(const float* qkv_dev, int64_t B, int32_t grid, int32_t S, int32_t num_heads, int32_t head_dim, const float* rel_h_dev,
                         const float* rel_w_dev, float* out_dev, void* stream) {
    WMAR_REQUIRE(qkv_dev && rel_h_dev && rel_w_dev && out_dev, "wamx_probe_attn: null argument");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && grid >= 1 && S >= 1 && num_heads >= 1 && num_heads <= 1024, "wamx_probe_attn: bad shape");
    hipStream_t st = (hipStream_t)stream;
    return probe_finish(run_wx_attn(qkv_dev, out_dev, rel_h_dev, rel_w_dev, (int)B, grid, S, num_heads, head_dim, st), st);
}

int wmar_wamx_probe_upstage(const float* x_dev, int64_t B, int32_t Hs, int32_t Cin, int32_t f, const float* ln_gamma_dev,
                            const float* ln_beta_dev, int32_t ln_gelu, const float* w_dev, int32_t Cout, float* out_dev, void* stream) {
    WMAR_REQUIRE(x_dev && w_dev && out_dev, "wamx_probe_upstage: null argument");
    WMAR_REQUIRE((ln_gamma_dev == nullptr) == (ln_beta_dev == nullptr), "wamx_probe_upstage: LayerNorm needs both gamma and beta");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && Hs >= 2 && Hs <= 4096 && Cin >= 1 && Cout >= 1 && (f == 2 || f == 4 || f == 8) && (Hs * f) % 8 == 0,
                 "wamx_probe_upstage: batch %lld (1..1024), size %d (>= 2), factor %d (2, 4 or 8; an output that is a multiple of 8), channels %d -> %d",
                 (long long)B, Hs, f, Cin, Cout);
    hipStream_t st = (hipStream_t)stream;
    DeviceArena mem;
    const char* names[3] = {"probe.weight", "ln.weight", "ln.bias"};
    const void* tensors[3] = {w_dev, ln_gamma_dev, ln_beta_dev};
    Loader ld(names, tensors, ln_gamma_dev ? 3 : 1, &mem, st);
    ConvW c;
    ld.conv("probe", Cin, Cout, 3, c, false);
    int& rc = ld.rc;
    WxLnRef ln{};
    if (ln_gamma_dev) {
        WxNorm n;
        float2* mr = nullptr;
        wx_load_norm(ld, "ln", Cin, n);
        WMAR_TRY(mem.alloc(&mr, (size_t)B * Hs * Hs));
        WMAR_TRY(run_wx_ln_stats(x_dev, mr, (long long)B * Hs * Hs, Cin, 1e-6f, st));
        ln = WxLnRef{mr, n.g, n.b, ln_gelu};
    }
    WMAR_TRY(run_wx_conv(WX_UPS, c, x_dev, out_dev, (int)B, Hs, f, ln_gamma_dev ? &ln : nullptr, nullptr, 0, 0, 0, 0, st));
    return probe_finish(rc, st);
}

int wmar_wamx_probe_last(const float* x_dev, int64_t B, int32_t H, int32_t Cin, const float* ln_gamma_dev, const float* ln_beta_dev,
                         int32_t ln_gelu, const float* w_dev, const float* bias_dev, int32_t Cout, float* out_dev, void* stream) {
    WMAR_REQUIRE(x_dev && w_dev && bias_dev && out_dev, "wamx_probe_last: null argument");
    WMAR_REQUIRE((ln_gamma_dev == nullptr) == (ln_beta_dev == nullptr), "wamx_probe_last: LayerNorm needs both gamma and beta");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && H >= 8 && H % 8 == 0 && H <= 4096 && Cin >= 1 && Cout >= 1,
                 "wamx_probe_last: batch %lld (1..1024), size %d (a multiple of 8), channels %d -> %d", (long long)B, H, Cin, Cout);
    hipStream_t st = (hipStream_t)stream;
    DeviceArena mem;
    const char* names[4] = {"probe.weight", "probe.bias", "ln.weight", "ln.bias"};
    const void* tensors[4] = {w_dev, bias_dev, ln_gamma_dev, ln_beta_dev};
    Loader ld(names, tensors, ln_gamma_dev ? 4 : 2, &mem, st);
    ConvW c;
    ld.conv("probe", Cin, Cout, 1, c);
    int& rc = ld.rc;
    WxLnRef ln{};
    if (ln_gamma_dev) {
        WxNorm n;
        float2* mr = nullptr;
        wx_load_norm(ld, "ln", Cin, n);
        WMAR_TRY(mem.alloc(&mr, (size_t)B * H * H));
        WMAR_TRY(run_wx_ln_stats(x_dev, mr, (long long)B * H * H, Cin, 1e-6f, st));
        ln = WxLnRef{mr, n.g, n.b, ln_gelu};
    }
    WMAR_TRY(run_wx_conv(WX_LN, c, x_dev, out_dev, (int)B, H, 1, ln_gamma_dev ? &ln : nullptr, nullptr, 0, 0, 1, 0, st));
    return probe_finish(rc, st);
}

int wmar_wamx_probe_block(wmar_wamx* w, int32_t block, const float* x_dev, int64_t B, float* out_dev, void* stream) {
    WMAR_REQUIRE(w && x_dev && out_dev, "wamx_probe_block: null argument");
    WMAR_REQUIRE(block >= 0 && block < w->cfg.depth && B >= 1 && B <= w->cfg.max_batch, "wamx_probe_block: block %d of %d, batch %lld (1..max_batch %d)",
                 block, w->cfg.depth, (long long)B, w->cfg.max_batch);
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)B * w->grid * w->grid * w->cfg.embed_dim * sizeof(float);
    int rc = WMAR_OK;
    if (hipMemcpyAsync(w->x, x_dev, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) { set_error("wamx_probe_block: copy in failed"); rc = WMAR_EHIP; }
    WMAR_TRY(wx_block(w, block, (int)B, st));
    if (rc == WMAR_OK && hipMemcpyAsync(out_dev, w->x, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        set_error("wamx_probe_block: copy out failed"); rc = WMAR_EHIP;
    }
    return probe_finish(rc, st);
}

}  // extern "C"
