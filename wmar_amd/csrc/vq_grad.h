// Backward of the Taming VQGAN layers (gfx950), one layer at a time: convolution (input, weight and bias gradients for the four
// index maps of the forward), GroupNorm (+ swish) and the attention core.  Included at the end of vqgan.hip: it shares that
// translation unit's packers, run_conv and the probe helpers, and adds no dispatch rule to the forward.
//
// Reference: deps/taming/modules/diffusionmodules/model.py:30-193 under torch.autograd (deps/taming/models/vqgan.py:86-169 trains
// through them).
//
// Conventions are the forward's: activations and their gradients NHWC fp32 with channels padded to a multiple of 8, weights and
// their gradients in torch layout [Cout][Cin][ks][ks].  No floating-point atomics: every reduction has a fixed order, two runs give
// the same bits.
//
//   dgrad   stride 1 (ks 1 or 3): a convolution of the output gradient with the spatially flipped, channel-transposed weight
//           (k_flip_transpose_w -> Loader::conv -> run_conv: the gradient rides the bf16-piece matrix path where the forward does).
//           `up`: that dgrad at 2H x 2W, then a 2 x 2 sum (the adjoint of nearest repetition).  Stride 2, zero pad (0, 1, 0, 1):
//           gather form, one thread per input element, taps outside and output channels inside (k_dgrad_s2).
//   wgrad   dW[co][ci][dy][dx] = sum over (b, oy, ox) of g[b][oy][ox][co] * y[b][iy][ix][ci]: an implicit GEMM with M = Cout,
//           N = Cin ks^2, K = B Ho Wo on v_mfma_f32_32x32x2_f32 (a k-ordered fp32 multiply-add chain per weight).  One wave owns a
//           32 x 32 (co, ci) tile for all taps of one K slice; K is split over workgroups, the slices' partial results go to a
//           workspace and k_fold_splits adds them in slice order.  The bias gradient is a two-stage sum the same way.
//   GroupNorm  per (image, chunk, channel) fp64 sums of dy and dy * xhat in fixed order (k_gnb_partial), folded per channel, per
//           (image, group) and over the batch (dgamma, dbeta), then the elementwise input gradient (k_gnb_apply).
//   attention  dV = P^T dO, dP = dO V^T, dS = scale P o (dP - rowsum(dP o P)), dQ = dS K, dK = dS^T Q with the taped softmax P.
//           The four products run as 1 x 1 convolutions with per-image packed weights (as attn_core's do) where that path takes the
//           shape, else through k_bmm_plain.
//   MaskGIT-VQGAN (RAR's tokenizer) adds three elementwise adjoints, all exact in fp32: the 2 x 2 average pool (k_avgpool2_bwd), and
//           the two image edges its fine-tuning differentiates -- clamp(v, 0, 1) * 2 - 1 behind the decoder (k_mvq_image_bwd) and
//           (x + 1) / 2 in front of the encoder (k_mvq_input_bwd).
#pragma once

namespace wmar {

// W [Cout][Cin][ks][ks] -> Wt [Cin][Cout][ks][ks], Wt[ci][co][dy][dx] = W[co][ci][ks-1-dy][ks-1-dx]
__global__ void k_flip_transpose_w(const float* __restrict__ W, float* __restrict__ Wt, int Cout, int Cin, int ks) {
    const int T = ks * ks;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)Cout * Cin * T) return;
    const int tap = (int)(idx % T);
    long long r = idx / T;
    const int co = (int)(r % Cout), ci = (int)(r / Cout);
    Wt[idx] = W[((long long)co * Cin + ci) * T + (T - 1 - tap)];
}

// in [B][2H][2W][C] -> out [B][H][W][C]: the sum of each 2 x 2 block, (top-left + top-right) + (bottom-left + bottom-right)
__global__ void k_sum2x2(const float* __restrict__ in, float* __restrict__ out, long long npix, int H, int W, int C) {
    const long long q4 = C >> 2;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * q4) return;
    const int c = (int)(idx % q4) * 4;
    const long long pix = idx / q4;
    const int x = (int)(pix % W);
    const long long t = pix / W;
    const int y = (int)(t % H);
    const long long b = t / H;
    const float* p = in + ((b * 2 * H + 2 * y) * (2LL * W) + 2 * x) * C + c;
    const float4 a = *(const float4*)p, b2 = *(const float4*)(p + C);
    const float4 c2 = *(const float4*)(p + 2LL * W * C), d = *(const float4*)(p + 2LL * W * C + C);
    *(float4*)(out + pix * C + c) = make_float4((a.x + b2.x) + (c2.x + d.x), (a.y + b2.y) + (c2.y + d.y), (a.z + b2.z) + (c2.z + d.z),
                                                (a.w + b2.w) + (c2.w + d.w));
}

// Adjoint of k_avgpool2 (MaskGIT-VQGAN downsampling), gather form: gy [B][Ho][Wo][C] -> gx [B][2Ho][2Wo][C], every input element
// takes a quarter of its window's gradient (g * 0.25f == g / 4 in fp32, what avg_pool2d's backward computes).
__global__ void k_avgpool2_bwd(const float* __restrict__ gy, float* __restrict__ gx, int Ho, int Wo, int C) {
    const long long q4 = C >> 2;
    const long long total = (long long)(2 * Ho) * (2 * Wo) * q4;
    const long long b = blockIdx.y;
    const float* gb = gy + b * (long long)Ho * Wo * C;
    float* xb = gx + b * (long long)(2 * Ho) * (2 * Wo) * C;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(e % q4) * 4;
        const long long pix = e / q4;
        const int ix = (int)(pix % (2 * Wo)), iy = (int)(pix / (2 * Wo));
        const float4 g = *(const float4*)(gb + ((long long)(iy >> 1) * Wo + (ix >> 1)) * C + c);
        *(float4*)(xb + pix * C + c) = make_float4(g.x * 0.25f, g.y * 0.25f, g.z * 0.25f, g.w * 0.25f);
    }
}

// Adjoint of k_nhwc_to_nchw_01 (clamp(v, 0, 1) * 2 - 1 on the decoder output): pre [B][HW][Cs] the taped value v in front of the clamp,
// g [B][C][HW] the image gradient -> out [B][HW][Cs] = 2 g where 0 <= v <= 1 (both bounds included, as torch.clamp's backward), else 0;
// padding channels 0.  One thread per pixel: the reads of g are coalesced per channel, pre and out move as float4.
__global__ void k_mvq_image_bwd(const float* __restrict__ pre, const float* __restrict__ g, float* __restrict__ out, int C, int HW, int Cs) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long b = blockIdx.y;
    if (idx >= HW) return;
    const float* p = pre + (b * HW + idx) * Cs;
    float* o = out + (b * HW + idx) * Cs;
    for (int c0 = 0; c0 < Cs; c0 += 4) {
        const float4 v4 = *(const float4*)(p + c0);
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
        float r[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = c0 + i;
            const float gv = c < C ? g[(b * C + c) * HW + idx] : 0.0f;
            r[i] = (c < C && v[i] >= 0.0f && v[i] <= 1.0f) ? 2.0f * gv : 0.0f;
        }
        *(float4*)(o + c0) = make_float4(r[0], r[1], r[2], r[3]);
    }
}

// Adjoint of k_nchw_to_nhwc01 ((x + 1) / 2 in front of the encoder): g [B][HW][Cs] -> out [B][C][HW] = g * 0.5f
__global__ void k_mvq_input_bwd(const float* __restrict__ g, float* __restrict__ out, int C, int HW, int Cs) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long b = blockIdx.y;
    if (idx >= HW) return;
    for (int c = 0; c < C; ++c) out[(b * C + c) * HW + idx] = g[(b * HW + idx) * Cs + c] * 0.5f;
}

// Adjoint of the 3 x 3 stride-2 convolution with zero pad (0, 1, 0, 1) (Downsample.forward): out[oy][ox] reads x[2 oy + dy][2 ox + dx],
// so input element (iy, ix, ci) collects g[(iy - dy) / 2][(ix - dx) / 2][co] w[co][ci][dy][dx] over the taps of matching parity.
// One thread per input element, one fp32 multiply-add chain (taps outside, output channels inside).
__global__ void k_dgrad_s2(const float* __restrict__ g, const float* __restrict__ W, float* __restrict__ gx, long long total, int H, int Wd,
                           int Cin, int Cin_s, int Cout, int Cout_s) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int ci = (int)(idx % Cin_s);
    const long long pix = idx / Cin_s;
    const int ix = (int)(pix % Wd);
    const long long t = pix / Wd;
    const int iy = (int)(t % H);
    const long long b = t / H;
    const int Ho = H / 2, Wo = Wd / 2;
    float acc = 0.f;
    if (ci < Cin) {
        for (int dy = 0; dy < 3; ++dy) {
            const int ty = iy - dy;
            if (ty < 0 || (ty & 1) || (ty >> 1) >= Ho) continue;
            for (int dx = 0; dx < 3; ++dx) {
                const int tx = ix - dx;
                if (tx < 0 || (tx & 1) || (tx >> 1) >= Wo) continue;
                const float* gp = g + ((b * Ho + (ty >> 1)) * Wo + (tx >> 1)) * Cout_s;
                const float* wp = W + (long long)ci * 9 + dy * 3 + dx;
                for (int co = 0; co < Cout; ++co) acc = fmaf(gp[co], wp[(long long)co * Cin * 9], acc);
            }
        }
    }
    gx[idx] = acc;
}

struct WgradArgs {
    const float* g;      // [B][Ho][Wo][Cout_s]: gradient of the conv's output
    const float* y;      // [B][Hs][Ws][Cin_s]: the conv's actual input (after GroupNorm + swish where the forward fused them)
    float* ws;           // [S][Cout * Cin * ks * ks]: one torch-layout partial result per K slice
    int Hs, Ws, Cin, Cin_s, Ho, Wo, Cout, Cout_s, stride, up, pad;
    int CT, CIT;         // 32-wide tiles of output / input channels
    int K, Kc;           // K = B Ho Wo products per weight, Kc (even) per slice
};

// One wave per (K slice, cout tile, cin tile), all ks^2 taps: per step two output pixels (one per lane half), A = g[pixel][co],
// B = y[pixel + tap][ci] -- both 128-byte runs of an NHWC row.  Out-of-range pixels, taps in the padding and channels beyond the
// stored ones contribute zeros; rows co >= Cout and columns ci >= Cin are never stored, so padding channels cannot reach a weight.
template <int KS>
__global__ __launch_bounds__(64) void k_wgrad(WgradArgs a) {
    constexpr int T = KS * KS;
    const int lane = threadIdx.x, j = lane & 31, half = lane >> 5;
    int bid = blockIdx.x;
    const int cit = bid % a.CIT; bid /= a.CIT;
    const int ct = bid % a.CT;
    const int s = bid / a.CT;
    const int co = ct * 32 + j, ci = cit * 32 + j;
    const bool co_ok = co < a.Cout_s, ci_ok = ci < a.Cin_s;
    const int Hc = a.up ? 2 * a.Hs : a.Hs, Wc = a.up ? 2 * a.Ws : a.Ws;
    const int HoWo = a.Ho * a.Wo;
    const int k0 = s * a.Kc, k1 = min(a.K, k0 + a.Kc);
    f32x16 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    for (int kk = k0; kk < k1; kk += 2) {
        const int p = kk + half;
        const bool valid = p < k1;
        const int pc = valid ? p : k0;
        const int b = pc / HoWo, rem = pc - b * HoWo;
        const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
        const float av = (valid && co_ok) ? a.g[(long long)pc * a.Cout_s + co] : 0.f;
        float bv[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            int iy = oy * a.stride + t / KS - a.pad, ix = ox * a.stride + t % KS - a.pad;
            const bool in = valid && ci_ok && iy >= 0 && iy < Hc && ix >= 0 && ix < Wc;
            if (a.up) { iy >>= 1; ix >>= 1; }
            bv[t] = in ? a.y[(((long long)b * a.Hs + iy) * a.Ws + ix) * a.Cin_s + ci] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[t], acc[t], 0, 0, 0);
    }
    // lane holds column ci and rows ct*32 + (r&3) + 8*(r>>2) + 4*half
    if (ci >= a.Cin) return;
    float* dst = a.ws + (long long)s * a.Cout * a.Cin * T;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row >= a.Cout) continue;
#pragma unroll
        for (int t = 0; t < T; ++t) dst[((long long)row * a.Cin + ci) * T + t] = acc[t][r];
    }
}

// out[i] = ws[0][i] + ws[1][i] + ... in slice order
__global__ void k_fold_splits(const float* __restrict__ ws, float* __restrict__ out, long long n, int S) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = ws[i];
    for (int s = 1; s < S; ++s) v += ws[(long long)s * n + i];
    out[i] = v;
}

// bias gradient, stage 1: ws[chunk][co] = sum of g over the chunk's pixels (8 pixel rows per workgroup, folded in row order)
__global__ __launch_bounds__(256) void k_bgrad_partial(const float* __restrict__ g, float* __restrict__ ws, int K, int nchunk, int Cout,
                                                       int Cout_s) {
    __shared__ float red[8][32];
    const int chunk = blockIdx.x, c = blockIdx.y * 32 + (threadIdx.x & 31), row = threadIdx.x >> 5;
    const int p0 = (int)((long long)chunk * K / nchunk), p1 = (int)((long long)(chunk + 1) * K / nchunk);
    float s = 0.f;
    if (c < Cout)
        for (int p = p0 + row; p < p1; p += 8) s += g[(long long)p * Cout_s + c];
    red[row][threadIdx.x & 31] = s;
    __syncthreads();
    if (row == 0 && c < Cout) {
        float t = red[0][threadIdx.x];
        for (int r = 1; r < 8; ++r) t += red[r][threadIdx.x];
        ws[(long long)chunk * Cout + c] = t;
    }
}

// ------------------------------------------------------------------------ GroupNorm (+ swish) backward
struct GnbArgs {
    const float* x;      // NHWC [B][HW][C]: the norm's input
    const float* gy;     // gradient of swish(GN(x)) (or of GN(x))
    const float2* mr;    // taped (mean, rstd) per [image][group]
    const float* gamma; const float* beta;
    double* part;        // [B][nchunk][C][2]: sums of dy and dy * xhat per channel
    double* chan;        // [B][C][2]: the same folded over the chunks
    float2* gs;          // [B][32]: (sum dy gamma, sum dy gamma xhat) / n per group
    float* gx;
    int HW, C, nchunk, swish;
};

// xhat and the gradient dy at the GroupNorm's output (behind the swish when there is one)
__device__ __forceinline__ void gnb_elem(float x, float gy, float2 m, float g, float bt, int swish, float& xh, float& dy) {
    xh = (x - m.x) * m.y;
    dy = gy;
    if (swish) {
        const float yv = xh * g + bt;
        const float sg = 1.0f / (1.0f + expf(-yv));
        dy = gy * (sg * (1.0f + yv * (1.0f - sg)));
    }
}

__global__ __launch_bounds__(256) void k_gnb_partial(GnbArgs a) {
    __shared__ double tmp[256][4][2];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int q4 = a.C >> 2, cpg = a.C / 32;
    const int p0 = (int)((long long)chunk * a.HW / a.nchunk), p1 = (int)((long long)(chunk + 1) * a.HW / a.nchunk);
    const int col = threadIdx.x % q4, prow = threadIdx.x / q4, pstep = 256 / q4;
    double s[4] = {0, 0, 0, 0}, sx[4] = {0, 0, 0, 0};
    const long long base = (long long)b * a.HW * a.C;
    if (prow < pstep) {
        const int c = col * 4;
        float gg[4], bb[4];
        float2 m[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { gg[i] = a.gamma[c + i]; bb[i] = a.beta[c + i]; m[i] = a.mr[b * 32 + (c + i) / cpg]; }
        for (int p = p0 + prow; p < p1; p += pstep) {
            const float4 xv = *(const float4*)(a.x + base + (long long)p * a.C + c);
            const float4 gv = *(const float4*)(a.gy + base + (long long)p * a.C + c);
            const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, gys[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float xh, dy;
                gnb_elem(xs[i], gys[i], m[i], gg[i], bb[i], a.swish, xh, dy);
                s[i] += (double)dy;
                sx[i] += prod_f64(dy, xh);      // never a v_fmac_f64 chain: common.h
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { tmp[threadIdx.x][i][0] = s[i]; tmp[threadIdx.x][i][1] = sx[i]; }
    __syncthreads();
    if (threadIdx.x < q4) {
        double* o = a.part + (((long long)b * a.nchunk + chunk) * a.C + threadIdx.x * 4) * 2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double t0 = 0, t1 = 0;
            for (int r = 0; r < pstep; ++r) { t0 += tmp[r * q4 + threadIdx.x][i][0]; t1 += tmp[r * q4 + threadIdx.x][i][1]; }
            o[i * 2] = t0; o[i * 2 + 1] = t1;
        }
    }
}

// chan[b][c] = part[b][0][c] + part[b][1][c] + ... (chunk order)
__global__ void k_gnb_chan(GnbArgs a, int B) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * a.C) return;
    const int b = idx / a.C, c = idx - b * a.C;
    double t0 = 0, t1 = 0;
    for (int k = 0; k < a.nchunk; ++k) {
        const double* p = a.part + (((long long)b * a.nchunk + k) * a.C + c) * 2;
        t0 += p[0]; t1 += p[1];
    }
    a.chan[(long long)idx * 2] = t0; a.chan[(long long)idx * 2 + 1] = t1;
}

// per (image, group): the two sums of the input gradient, gamma-weighted in channel order, divided by the group's element count
__global__ void k_gnb_group(GnbArgs a) {
    const int b = blockIdx.x, g = threadIdx.x;
    const int cpg = a.C / 32;
    double s1 = 0, s2 = 0;
    for (int i = 0; i < cpg; ++i) {
#pragma clang fp contract(off)
        const int c = g * cpg + i;
        double p1 = (double)a.gamma[c] * a.chan[((long long)b * a.C + c) * 2];
        double p2 = (double)a.gamma[c] * a.chan[((long long)b * a.C + c) * 2 + 1];
        asm volatile("" : "+v"(p1));      // products kept out of a fused multiply-add chain: common.h
        asm volatile("" : "+v"(p2));
        s1 += p1; s2 += p2;
    }
    const double rn = inv_count_f64((double)a.HW * cpg);
    a.gs[b * 32 + g] = make_float2((float)(s1 * rn), (float)(s2 * rn));
}

// dbeta[c] = sum over images of sum dy, dgamma[c] = sum over images of sum dy * xhat (image order)
__global__ void k_gnb_param(GnbArgs a, int B, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C) return;
    double t0 = 0, t1 = 0;
    for (int b = 0; b < B; ++b) { t0 += a.chan[((long long)b * a.C + c) * 2]; t1 += a.chan[((long long)b * a.C + c) * 2 + 1]; }
    dbeta[c] = (float)t0; dgamma[c] = (float)t1;
}

// g_x = rstd (dy gamma - mean_g(dy gamma) - xhat mean_g(dy gamma xhat))
__global__ void k_gnb_apply(GnbArgs a, long long total4) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total4) return;
    const int q4 = a.C >> 2, cpg = a.C / 32;
    const int c = (int)(idx % q4) * 4;
    const long long pix = idx / q4;
    const int b = (int)(pix / a.HW);
    const float4 xv = *(const float4*)(a.x + pix * a.C + c);
    const float4 gv = *(const float4*)(a.gy + pix * a.C + c);
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, gys[4] = {gv.x, gv.y, gv.z, gv.w};
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int grp = b * 32 + (c + i) / cpg;
        const float2 m = a.mr[grp], sn = a.gs[grp];
        const float g = a.gamma[c + i];
        float xh, dy;
        gnb_elem(xs[i], gys[i], m, g, a.beta[c + i], a.swish, xh, dy);
        o[i] = m.y * ((dy * g - sn.x) - xh * sn.y);
    }
    *(float4*)(a.gx + pix * a.C + c) = make_float4(o[0], o[1], o[2], o[3]);
}

// ------------------------------------------------------------------------ attention backward
// per image (blockIdx.y): in [R][Cc] -> out [Cc][R]
__global__ void k_transpose_img(const float* __restrict__ in, float* __restrict__ out, int R, int Cc) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)R * Cc) return;
    const long long off = (long long)blockIdx.y * R * Cc;
    const int r = (int)(idx / Cc), c = (int)(idx - (long long)r * Cc);
    out[off + (long long)c * R + r] = in[off + idx];
}

// dS = scale P o (dP - rowsum(dP o P)), in place over dP: one wave per row, lane partial sums folded by a fixed butterfly
__global__ __launch_bounds__(256) void k_attn_softmax_bwd(const float* __restrict__ P, float* __restrict__ dP, long long rows, int N,
                                                          float scale) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = P + row * N;
    float* d = dP + row * N;
    float sum = 0.f;
    for (int j = lane; j < N; j += 64) sum += d[j] * p[j];
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    for (int j = lane; j < N; j += 64) d[j] = scale * (p[j] * (d[j] - sum));
}

// out[b][m][n] = sum_k A[b][m sa_m + k sa_k] Bm[b][k sb_k + n sb_n]: one thread per output, one fp32 multiply-add chain (the shapes
// the matrix path rejects)
__global__ void k_bmm_plain(const float* __restrict__ A, const float* __restrict__ Bm, float* __restrict__ out, int M, int Nn, int Kk,
                            long long sa_m, long long sa_k, long long sb_k, long long sb_n, long long a_b, long long b_b) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)M * Nn) return;
    const int m = (int)(idx / Nn), n = (int)(idx - (long long)m * Nn);
    const float* ap = A + blockIdx.y * a_b + m * sa_m;
    const float* bp = Bm + blockIdx.y * b_b + n * sb_n;
    float acc = 0.f;
    for (int k = 0; k < Kk; ++k) acc = fmaf(ap[k * sa_k], bp[k * sb_k], acc);
    out[(long long)blockIdx.y * M * Nn + idx] = acc;
}

}  // namespace wmar

namespace {

// what the last backward call on this thread launched (reported by the wmar_vq_probe_*_backward entries)
static thread_local char g_dgrad_path[96] = "none";
static thread_local const char* g_wgrad_kernel = "none";
static thread_local int g_wgrad_splits = 0;
static thread_local const char* g_attnb_path = "none";

constexpr int WGRAD_K_MIN = 256;        // products per weight below which a K slice is not split further
constexpr int WGRAD_WAVES = 1024;       // target number of waves (256 CUs x 4 SIMDs)
constexpr int WGRAD_SPLITS_MAX = 64;

inline int wgrad_splits(int K, int cout, int cin) {
    const int tiles = ((cout + 31) / 32) * ((cin + 31) / 32);
    int S = (K + WGRAD_K_MIN - 1) / WGRAD_K_MIN;
    const int fill = (WGRAD_WAVES + tiles - 1) / tiles;
    if (S > fill) S = fill;
    if (S > WGRAD_SPLITS_MAX) S = WGRAD_SPLITS_MAX;
    return S < 1 ? 1 : S;
}
inline int bgrad_chunks(int K) { int n = K / 512; return n < 1 ? 1 : (n > 128 ? 128 : n); }
// floats of workspace run_conv_wgrad needs
inline size_t wgrad_ws_elems(int K, int cout, int cin, int ks) {
    return (size_t)wgrad_splits(K, cout, cin) * cout * cin * ks * ks + (size_t)bgrad_chunks(K) * cout;
}

// The dgrad "convolution" of a stride-1 conv: the flipped, transposed weight packed by the forward's loader (zero bias).
int make_dgrad_conv(DeviceArena& mem, const float* w, int cout, int cin, int ks, hipStream_t st, ConvW* out) {
    float* wt = nullptr;
    if (int rc = mem.alloc(&wt, (size_t)cout * cin * ks * ks)) return rc;
    const long long n = (long long)cout * cin * ks * ks;
    hipLaunchKernelGGL(k_flip_transpose_w, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, wt, cout, cin, ks);
    if (int rc = launch_status("k_flip_transpose_w")) return rc;
    const char* names[1] = {"dgrad.weight"};
    const void* tensors[1] = {wt};
    Loader ld(names, tensors, 1, &mem, st);
    ld.conv("dgrad", cout, cin, ks, *out, false);
    return ld.rc;
}

// g_x of a conv.  dg: make_dgrad_conv's result (stride 1), w: the raw weight (stride 2); gy [B][Ho][Wo][cout_s] -> gx [B][Hs][Ws][cin_s];
// up_scratch [B][2Hs][2Ws][cin_s] when up.
int run_conv_dgrad(const ConvW* dg, const float* w, int cout, int cin, int ks, const float* gy, float* gx, float* up_scratch, int B, int Hs,
                   int Ws, int stride, int up, hipStream_t st) {
    int rc;
    if (stride == 2) {
        WMAR_REQUIRE(ks == 3 && !up && Hs % 2 == 0 && Ws % 2 == 0, "conv dgrad: stride 2 is 3 x 3 without upsampling, even size");
        const long long total = (long long)B * Hs * Ws * pad8(cin);
        hipLaunchKernelGGL(k_dgrad_s2, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, gy, w, gx, total, Hs, Ws, cin, pad8(cin),
                           cout, pad8(cout));
        snprintf(g_dgrad_path, sizeof g_dgrad_path, "k_dgrad_s2");
        return launch_status("k_dgrad_s2");
    }
    WMAR_REQUIRE(dg && dg->cin == cout && dg->cout == cin, "conv dgrad: the flipped weight does not belong to this conv");
    if (!up) {
        if ((rc = run_conv(*dg, gy, gx, nullptr, B, Hs, Ws, 1, 0, st))) return rc;
        snprintf(g_dgrad_path, sizeof g_dgrad_path, "flip+%s", g_conv_kernel);
        return WMAR_OK;
    }
    WMAR_REQUIRE(up_scratch, "conv dgrad: upsampling needs scratch");
    if ((rc = run_conv(*dg, gy, up_scratch, nullptr, B, 2 * Hs, 2 * Ws, 1, 0, st))) return rc;
    const long long npix = (long long)B * Hs * Ws;
    const int Cs = pad8(cin);
    hipLaunchKernelGGL(k_sum2x2, dim3((unsigned)((npix * (Cs / 4) + 255) / 256)), dim3(256), 0, st, (const float*)up_scratch, gx, npix, Hs,
                       Ws, Cs);
    snprintf(g_dgrad_path, sizeof g_dgrad_path, "flip+%s+k_sum2x2", g_conv_kernel);
    return launch_status("k_sum2x2");
}

// g_w [cout][cin][ks][ks] and g_b [cout] (nullable) of a conv from gy [B][Ho][Wo][cout_s] and the conv's actual input y
// [B][Hs][Ws][cin_s]; ws: wgrad_ws_elems floats.
int run_conv_wgrad(const float* gy, const float* y, float* gw, float* gb, float* ws, int cout, int cin, int ks, int B, int Hs, int Ws,
                   int stride, int up, hipStream_t st) {
    WgradArgs a{};
    const int Hc = up ? 2 * Hs : Hs, Wc = up ? 2 * Ws : Ws;
    a.g = gy; a.y = y; a.ws = ws;
    a.Hs = Hs; a.Ws = Ws; a.Cin = cin; a.Cin_s = pad8(cin); a.Cout = cout; a.Cout_s = pad8(cout);
    a.Ho = stride == 2 ? Hc / 2 : Hc; a.Wo = stride == 2 ? Wc / 2 : Wc;
    a.stride = stride; a.up = up; a.pad = (ks == 3 && stride == 1) ? 1 : 0;
    a.CT = (cout + 31) / 32; a.CIT = (cin + 31) / 32;
    const long long K = (long long)B * a.Ho * a.Wo;
    WMAR_REQUIRE(K >= 1 && K < (1LL << 30), "conv wgrad: %lld output pixels", K);
    a.K = (int)K;
    const int S = wgrad_splits(a.K, cout, cin);
    a.Kc = ((a.K + S - 1) / S + 1) & ~1;
    const unsigned grid = (unsigned)((long long)S * a.CT * a.CIT);
    if (ks == 3) { g_wgrad_kernel = "k_wgrad<3>"; hipLaunchKernelGGL(k_wgrad<3>, dim3(grid), dim3(64), 0, st, a); }
    else { g_wgrad_kernel = "k_wgrad<1>"; hipLaunchKernelGGL(k_wgrad<1>, dim3(grid), dim3(64), 0, st, a); }
    g_wgrad_splits = S;
    const long long n = (long long)cout * cin * ks * ks;
    hipLaunchKernelGGL(k_fold_splits, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)ws, gw, n, S);
    if (gb) {
        float* wb = ws + (size_t)S * n;
        const int nchunk = bgrad_chunks(a.K);
        hipLaunchKernelGGL(k_bgrad_partial, dim3(nchunk, a.CT), dim3(256), 0, st, gy, wb, a.K, nchunk, cout, a.Cout_s);
        hipLaunchKernelGGL(k_fold_splits, dim3((cout + 255) / 256), dim3(256), 0, st, (const float*)wb, gb, (long long)cout, nchunk);
    }
    return launch_status("k_wgrad");
}

inline int gnb_chunks(int HW) { int n = HW / 256; return n < 1 ? 1 : (n > GN_CHUNKS_MAX ? GN_CHUNKS_MAX : n); }
// doubles of scratch run_gn_backward needs
inline size_t gnb_scratch_doubles(int B, int HW, int C) { return (size_t)B * gnb_chunks(HW) * C * 2 + (size_t)B * C * 2 + (size_t)B * 32; }

// GroupNorm(32, eps 1e-6) (+ swish) backward: x, gy, gx NHWC [B][HW][C] (C a multiple of 32), mr the forward's (mean, rstd).
int run_gn_backward(const float* x, const float* gy, const float2* mr, const float* gamma, const float* beta, int C, int B, int HW, int swish,
                    double* scratch, float* gx, float* dgamma, float* dbeta, hipStream_t st) {
    WMAR_REQUIRE(C % 32 == 0 && C / 4 <= 256, "GroupNorm backward: channel count %d unsupported (multiple of 32, <= 1024)", C);
    GnbArgs a{};
    a.x = x; a.gy = gy; a.mr = mr; a.gamma = gamma; a.beta = beta; a.gx = gx; a.HW = HW; a.C = C; a.swish = swish;
    a.nchunk = gnb_chunks(HW);
    a.part = scratch;
    a.chan = scratch + (size_t)B * a.nchunk * C * 2;
    a.gs = (float2*)(a.chan + (size_t)B * C * 2);
    hipLaunchKernelGGL(k_gnb_partial, dim3(a.nchunk, B), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_gnb_chan, dim3((B * C + 255) / 256), dim3(256), 0, st, a, B);
    hipLaunchKernelGGL(k_gnb_group, dim3(B), dim3(32), 0, st, a);
    hipLaunchKernelGGL(k_gnb_param, dim3((C + 255) / 256), dim3(256), 0, st, a, B, dgamma, dbeta);
    const long long total4 = (long long)B * HW * (C / 4);
    hipLaunchKernelGGL(k_gnb_apply, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, a, total4);
    return launch_status("k_gnb");
}

// 2 x 2 average pool backward: gy [B][Ho][Wo][C] -> gx [B][2Ho][2Wo][C]; the grid is k_avgpool2's rule on the input-sized tensor
int run_avgpool_backward(const float* gy, float* gx, int B, int Ho, int Wo, int C, hipStream_t st) {
    WMAR_REQUIRE(C % 4 == 0, "average pool backward: channel count %d is not a multiple of 4", C);
    const long long total = (long long)(2 * Ho) * (2 * Wo) * (C / 4);
    int gx_ = (int)((total + 255) / 256);
    if (gx_ > 8192) gx_ = 8192;
    hipLaunchKernelGGL(k_avgpool2_bwd, dim3(gx_, (unsigned)B), dim3(256), 0, st, gy, gx, Ho, Wo, C);
    return launch_status("k_avgpool2_bwd");
}

// the two image edges of the MaskGIT-VQGAN halves (k_mvq_image_bwd, k_mvq_input_bwd)
int run_mvq_image_backward(const float* pre, const float* g_nchw, float* g_nhwc, int B, int C, int HW, int Cs, hipStream_t st) {
    WMAR_REQUIRE(Cs % 4 == 0 && C <= Cs, "image backward: %d channels stored as %d", C, Cs);
    hipLaunchKernelGGL(k_mvq_image_bwd, dim3((HW + 255) / 256, (unsigned)B), dim3(256), 0, st, pre, g_nchw, g_nhwc, C, HW, Cs);
    return launch_status("k_mvq_image_bwd");
}
int run_mvq_input_backward(const float* g_nhwc, float* g_nchw, int B, int C, int HW, int Cs, hipStream_t st) {
    WMAR_REQUIRE(C <= Cs, "input backward: %d channels stored as %d", C, Cs);
    hipLaunchKernelGGL(k_mvq_input_bwd, dim3((HW + 255) / 256, (unsigned)B), dim3(256), 0, st, g_nhwc, g_nchw, C, HW, Cs);
    return launch_status("k_mvq_input_bwd");
}

// Backward of attn_core with the taped softmax P [B][N][N]: dO -> dQ, dK, dV (all [B][N][C]).  dp, tr: [B][N][N] floats of scratch
// each; s.attk / s.attv / s.zbias as attn_core takes them.
int attn_backward(const AttnScratch& s, float* dp, float* tr, const float* q, const float* k, const float* vv, const float* P, const float* dO,
                  float* dq, float* dk, float* dv, int B, int H, int W, int C, hipStream_t st) {
    int rc;
    const int N = H * W;
    const float scale = 1.0f / sqrtf((float)C);
    const long long NN = (long long)N * N, NC = (long long)N * C;
    const unsigned gNN = (unsigned)((NN + 255) / 256), gNC = (unsigned)((NC + 255) / 256);
    const unsigned grows = (unsigned)(((long long)B * N + 3) / 4);
    if (s.attk && N % 32 == 0 && C % 32 == 0 && H % 8 == 0 && W % 8 == 0 && N >= 64 && C >= 64 && !conv_no_bx()) {
        // per-image weights on the bf16 matrix pipe, as attn_core: c_nc has N output "channels" over C inputs, c_cn the reverse
        ConvW c_nc{}, c_cn{};
        c_nc.bias = s.zbias; c_nc.cin = c_nc.cin_s = C; c_nc.cout = c_nc.cout_s = N; c_nc.ks = 1; c_nc.CT = N / 32; c_nc.KBc = C / 8;
        c_cn.bias = s.zbias; c_cn.cin = c_cn.cin_s = N; c_cn.cout = c_cn.cout_s = C; c_cn.ks = 1; c_cn.CT = C / 32; c_cn.KBc = N / 8;
        const long long s_nc = (long long)c_nc.CT * (C / 16) * 192, s_cn = (long long)c_cn.CT * (N / 16) * 192;
        const long long n_nc = (long long)c_nc.CT * (C / 16) * 64, n_cn = (long long)c_cn.CT * (N / 16) * 64;
        const unsigned g_nc = (unsigned)((n_nc + 255) / 256), g_cn = (unsigned)((n_cn + 255) / 256);
        // dP[i][j] = sum_c dO[i][c] V[j][c]
        c_nc.wq = s.attk;
        hipLaunchKernelGGL(k_pack_conv_bx, dim3(g_nc, B), dim3(256), 0, st, vv, s.attk, N, C, 1, c_nc.CT, C / 16, NC, s_nc, 0);
        if ((rc = run_conv(c_nc, dO, dp, nullptr, B, H, W, 1, 0, st, nullptr, s_nc))) return rc;
        // dV[j][c] = sum_i P[i][j] dO[i][c]
        hipLaunchKernelGGL(k_transpose_img, dim3(gNN, B), dim3(256), 0, st, P, tr, N, N);
        c_cn.wq = s.attv;
        hipLaunchKernelGGL(k_pack_conv_bx, dim3(g_cn, B), dim3(256), 0, st, dO, s.attv, C, N, 1, c_cn.CT, N / 16, NC, s_cn, 1);
        if ((rc = run_conv(c_cn, tr, dv, nullptr, B, H, W, 1, 0, st, nullptr, s_cn))) return rc;
        hipLaunchKernelGGL(k_attn_softmax_bwd, dim3(grows), dim3(256), 0, st, P, dp, (long long)B * N, N, scale);
        // dQ[i][c] = sum_j dS[i][j] K[j][c]
        c_cn.wq = s.attk;
        hipLaunchKernelGGL(k_pack_conv_bx, dim3(g_cn, B), dim3(256), 0, st, k, s.attk, C, N, 1, c_cn.CT, N / 16, NC, s_cn, 1);
        if ((rc = run_conv(c_cn, dp, dq, nullptr, B, H, W, 1, 0, st, nullptr, s_cn))) return rc;
        // dK[j][c] = sum_i dS[i][j] Q[i][c]
        hipLaunchKernelGGL(k_transpose_img, dim3(gNN, B), dim3(256), 0, st, (const float*)dp, tr, N, N);
        c_cn.wq = s.attv;
        hipLaunchKernelGGL(k_pack_conv_bx, dim3(g_cn, B), dim3(256), 0, st, q, s.attv, C, N, 1, c_cn.CT, N / 16, NC, s_cn, 1);
        if ((rc = run_conv(c_cn, tr, dk, nullptr, B, H, W, 1, 0, st, nullptr, s_cn))) return rc;
        g_attnb_path = "bf16_pipe";
    } else {
        hipLaunchKernelGGL(k_bmm_plain, dim3(gNN, B), dim3(256), 0, st, dO, vv, dp, N, N, C, (long long)C, 1LL, 1LL, (long long)C, NC, NC);
        hipLaunchKernelGGL(k_bmm_plain, dim3(gNC, B), dim3(256), 0, st, P, dO, dv, N, C, N, 1LL, (long long)N, (long long)C, 1LL, NN, NC);
        hipLaunchKernelGGL(k_attn_softmax_bwd, dim3(grows), dim3(256), 0, st, P, dp, (long long)B * N, N, scale);
        hipLaunchKernelGGL(k_bmm_plain, dim3(gNC, B), dim3(256), 0, st, (const float*)dp, k, dq, N, C, N, (long long)N, 1LL, (long long)C, 1LL, NN, NC);
        hipLaunchKernelGGL(k_bmm_plain, dim3(gNC, B), dim3(256), 0, st, (const float*)dp, q, dk, N, C, N, 1LL, (long long)N, (long long)C, 1LL, NN, NC);
        g_attnb_path = "plain";
    }
    return launch_status("attention backward");
}

}  // namespace

// ------------------------------------------------------------------------------ probes (tests, debugging)
extern "C" {

int wmar_vq_probe_conv_backward(const float* w_dev, int32_t cout, int32_t cin, int32_t ks, const float* x_dev, const float* gy_dev, int64_t B,
                                int32_t Hs, int32_t Ws, int32_t stride, int32_t up, float* gx_dev, float* gw_dev, float* gb_dev,
                                char* kernel_buf, int64_t buf_len, void* stream) {
    WMAR_REQUIRE(w_dev && x_dev && gy_dev && gx_dev && gw_dev && kernel_buf && buf_len > 0, "vq_probe_conv_backward: null argument");
    WMAR_REQUIRE(cout >= 1 && cin >= 1 && (ks == 1 || ks == 3) && B >= 1 && B <= 1024 && Hs >= 1 && Ws >= 1, "vq_probe_conv_backward: bad shape");
    WMAR_REQUIRE(stride == 1 || (stride == 2 && ks == 3 && !up), "vq_probe_conv_backward: stride %d (2 only for 3 x 3 without upsampling)", stride);
    hipStream_t st = (hipStream_t)stream;
    DeviceArena mem;
    int rc = WMAR_OK;
    g_trk = GnTrack{};
    const int Hc = up ? 2 * Hs : Hs, Wc = up ? 2 * Ws : Ws;
    const int Ho = stride == 2 ? Hc / 2 : Hc, Wo = stride == 2 ? Wc / 2 : Wc;
    const long long K64 = (long long)B * Ho * Wo;
    WMAR_REQUIRE(Ho >= 1 && Wo >= 1 && K64 < (1LL << 30) && (long long)B * Hc * Wc * pad8(cin) < (1LL << 40),
                 "vq_probe_conv_backward: %lld output pixels are beyond what the weight gradient indexes", K64);
    ConvW dg;
    float *ups = nullptr, *ws = nullptr;
    if (stride == 1) WMAR_TRY(make_dgrad_conv(mem, w_dev, cout, cin, ks, st, &dg));
    if (up) WMAR_TRY(mem.alloc(&ups, (size_t)B * Hc * Wc * pad8(cin)));
    // The workspace always has the size a conv with a bias needs and starts as all-ones bytes (a NaN pattern no sum produces): a
    // bias-free call (gb_dev null, the MaskGIT plan's convs) must leave the bias part of it as it was.
    const size_t ws_elems = wgrad_ws_elems((int)K64, cout, cin, ks);
    const size_t tail = (size_t)bgrad_chunks((int)K64) * cout;
    WMAR_TRY(mem.alloc(&ws, ws_elems));
    if (rc == WMAR_OK && hipMemsetAsync(ws, 0xff, ws_elems * sizeof(float), st) != hipSuccess) {
        set_error("vq_probe_conv_backward: workspace memset failed"); rc = WMAR_EHIP;
    }
    WMAR_TRY(run_conv_dgrad(stride == 1 ? &dg : nullptr, w_dev, cout, cin, ks, gy_dev, gx_dev, ups, (int)B, Hs, Ws, stride, up, st));
    WMAR_TRY(run_conv_wgrad(gy_dev, x_dev, gw_dev, gb_dev, ws, cout, cin, ks, (int)B, Hs, Ws, stride, up, st));
    if (rc == WMAR_OK && !gb_dev) {
        std::vector<uint32_t> host(tail);
        const hipError_t e = hipMemcpyAsync(host.data(), ws + (ws_elems - tail), tail * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { set_error("vq_probe_conv_backward: reading the workspace back failed"); rc = WMAR_EHIP; }
        for (size_t i = 0; rc == WMAR_OK && i < tail; ++i)
            if (host[i] != 0xffffffffu) {
                set_error("vq_probe_conv_backward: a bias-free weight gradient wrote the bias workspace (element %zu of %zu)", i, tail);
                rc = WMAR_EINVAL;
            }
    }
    if (rc == WMAR_OK) {
        const int n = snprintf(kernel_buf, (size_t)buf_len, "dgrad=%s;wgrad=%s;splits=%d;bgrad=%s", g_dgrad_path, g_wgrad_kernel, g_wgrad_splits,
                               gb_dev ? "k_bgrad_partial" : "none");
        if (!(n > 0 && n < buf_len)) { set_error("vq_probe_conv_backward: buffer of %lld bytes too small", (long long)buf_len); rc = WMAR_EINVAL; }
    }
    return probe_finish(rc, st);
}

int wmar_vq_probe_gn_backward(const float* x_dev, const float* gy_dev, const float* mr_dev, const float* gamma_dev, const float* beta_dev,
                              int64_t B, int32_t HW, int32_t C, int32_t swish, float* gx_dev, float* dgamma_dev, float* dbeta_dev,
                              char* path_buf, int64_t buf_len, void* stream) {
    WMAR_REQUIRE(x_dev && gy_dev && mr_dev && gamma_dev && beta_dev && gx_dev && dgamma_dev && dbeta_dev && path_buf && buf_len > 0,
                 "vq_probe_gn_backward: null argument");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && HW >= 1 && C >= 32, "vq_probe_gn_backward: bad shape");
    hipStream_t st = (hipStream_t)stream;
    DeviceArena mem;
    int rc = WMAR_OK;
    double* scratch = nullptr;
    WMAR_TRY(mem.alloc(&scratch, gnb_scratch_doubles((int)B, HW, C)));
    WMAR_TRY(run_gn_backward(x_dev, gy_dev, (const float2*)mr_dev, gamma_dev, beta_dev, C, (int)B, HW, swish, scratch, gx_dev, dgamma_dev,
                             dbeta_dev, st));
    if (rc == WMAR_OK) {
        const int n = snprintf(path_buf, (size_t)buf_len, "path=k_gnb_partial+k_gnb_apply;chunks=%d", gnb_chunks(HW));
        if (!(n > 0 && n < buf_len)) { set_error("vq_probe_gn_backward: buffer of %lld bytes too small", (long long)buf_len); rc = WMAR_EINVAL; }
    }
    return probe_finish(rc, st);
}

int wmar_vq_probe_attn_backward(const float* q_dev, const float* k_dev, const float* v_dev, const float* go_dev, int64_t B, int32_t H, int32_t W,
                                int32_t C, float* gq_dev, float* gk_dev, float* gv_dev, char* path_buf, int64_t buf_len, void* stream) {
    WMAR_REQUIRE(q_dev && k_dev && v_dev && go_dev && gq_dev && gk_dev && gv_dev && path_buf && buf_len > 0, "vq_probe_attn_backward: null argument");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0 && C <= 1024, "vq_probe_attn_backward: bad shape");
    hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)H * W;
    DeviceArena mem;
    AttnScratch s{};
    float *o = nullptr, *dp = nullptr, *tr = nullptr;
    int rc = WMAR_OK;
    g_trk = GnTrack{};
    WMAR_TRY(mem.alloc(&s.asc, (size_t)B * N * N));
    WMAR_TRY(mem.alloc(&dp, (size_t)B * N * N));
    WMAR_TRY(mem.alloc(&tr, (size_t)B * N * N));
    WMAR_TRY(mem.alloc(&o, (size_t)B * N * C));
    if (N % 32 == 0 && C % 32 == 0) {      // as wmar_vq_create sizes them
        WMAR_TRY(mem.alloc(&s.attk, (size_t)B * N * C * 3 / 8));
        WMAR_TRY(mem.alloc(&s.attv, (size_t)B * N * C * 3 / 8));
        WMAR_TRY(mem.alloc_zero(&s.zbias, N > (size_t)C ? N : (size_t)C, st));
    }
    // the forward leaves the softmax in s.asc: that is the tape
    WMAR_TRY(attn_core(s, q_dev, k_dev, v_dev, o, (int)B, H, W, C, st));
    WMAR_TRY(attn_backward(s, dp, tr, q_dev, k_dev, v_dev, s.asc, go_dev, gq_dev, gk_dev, gv_dev, (int)B, H, W, C, st));
    if (rc == WMAR_OK) {
        const int n = snprintf(path_buf, (size_t)buf_len, "path=%s;forward=%s", g_attnb_path, g_attn_path);
        if (!(n > 0 && n < buf_len)) { set_error("vq_probe_attn_backward: buffer of %lld bytes too small", (long long)buf_len); rc = WMAR_EINVAL; }
    }
    return probe_finish(rc, st);
}

int wmar_vq_probe_avgpool_backward(const float* gy_dev, int64_t B, int32_t Ho, int32_t Wo, int32_t C, float* gx_dev, void* stream) {
    WMAR_REQUIRE(gy_dev && gx_dev, "vq_probe_avgpool_backward: null argument");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && Ho >= 1 && Wo >= 1 && C >= 4 && C % 4 == 0 && (long long)B * Ho * Wo * C < (1LL << 38),
                 "vq_probe_avgpool_backward: bad shape");
    hipStream_t st = (hipStream_t)stream;
    return probe_finish(run_avgpool_backward(gy_dev, gx_dev, (int)B, Ho, Wo, C, st), st);
}

int wmar_mvq_probe_image_backward(const float* pre_dev, const float* g_nchw_dev, int64_t B, int32_t C, int32_t HW, int32_t Cs, float* g_nhwc_dev,
                                  void* stream) {
    WMAR_REQUIRE(pre_dev && g_nchw_dev && g_nhwc_dev, "mvq_probe_image_backward: null argument");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && C >= 1 && HW >= 1 && Cs >= C && Cs % 4 == 0, "mvq_probe_image_backward: bad shape");
    hipStream_t st = (hipStream_t)stream;
    return probe_finish(run_mvq_image_backward(pre_dev, g_nchw_dev, g_nhwc_dev, (int)B, C, HW, Cs, st), st);
}

int wmar_mvq_probe_input_backward(const float* g_nhwc_dev, int64_t B, int32_t C, int32_t HW, int32_t Cs, float* g_nchw_dev, void* stream) {
    WMAR_REQUIRE(g_nhwc_dev && g_nchw_dev, "mvq_probe_input_backward: null argument");
    WMAR_REQUIRE(B >= 1 && B <= 1024 && C >= 1 && HW >= 1 && Cs >= C, "mvq_probe_input_backward: bad shape");
    hipStream_t st = (hipStream_t)stream;
    return probe_finish(run_mvq_input_backward(g_nhwc_dev, g_nchw_dev, (int)B, C, HW, Cs, st), st);
}

}  // extern "C"
