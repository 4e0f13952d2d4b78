// Evaluation transforms of the harness as HIP kernels over the WHOLE batch: Gaussian blur, Gaussian noise,
// brightness, rotation, horizontal flip, upper-left crop + resize back / pad back.
//
// Reference: wmar/augmentations/valuemetric.py:41-140, geometric.py:22-117 (modules that delegate to
// torchvision.transforms.functional), applied by generate.py:142-164 to every generated batch: ~90 (transform, parameter) pairs per
// image, each followed by images_to_codes + detect.  The arithmetic restated here is the PUBLISHED torchvision tensor algorithm of
// each call (torchvision is not installed offline; tests/test_augmentations_algorithms.py holds independent numpy restatements):
//   gaussian_blur(img, k)      separable weights exp(-x^2 / 2 s^2), s = 0.3 ((k - 1) / 2 - 1) + 0.8, normalised; reflect padding;
//                              depthwise 2-D correlation with w[i] w[j]
//   adjust_brightness(img, f)  f * img clamped to [0, 1]
//   rotate(img, angle)         quarter turns as an exact permutation (geometric.py:38-46), the rest as the inverse affine map about the
//                              image centre in pixel-centre coordinates, nearest sample (round half to even), zero fill
//   resize(antialias=True)     separable triangle filter widened by the scale factor, normalised weights
// One pass per transform: with `pm1` the kernel reads the decoder's [-1, 1] pixels, works in [0, 1], clamps and writes [-1, 1] again
// (the harness's `aug(imgs / 2 + 0.5).clamp(0, 1) * 2 - 1`, generate.py:146-150, bit for bit: x / 2 and c * 2 are exact).
#include "common.h"

namespace wmar {

enum { AUG_IDENTITY = 0, AUG_BLUR = 1, AUG_NOISE = 2, AUG_BRIGHTNESS = 3, AUG_ROTATE = 4, AUG_FLIP_H = 5, AUG_CROP_RESIZE = 6, AUG_CROP_PAD = 7 };
constexpr int AUG_MAX_K = 63;

struct AugArgs {
    const float* in;
    float* out;
    const float* noise;     // AUG_NOISE: standard normal draws, same shape as the images
    int planes, H, W;       // planes = B * C
    int pm1;
    int k;                  // blur: odd kernel size
    float w[AUG_MAX_K];     // blur: 1-D weights
    float f;                // brightness factor / noise standard deviation
    float cs, sn;           // rotation: cos / sin of the remainder angle
    int quarters;           // rotation: counter-clockwise quarter turns applied first (0..3)
    int has_rest;           // rotation: remainder != 0
    int nh, nw;             // crop: kept rows / columns
};

__device__ __forceinline__ float aug_in(const AugArgs& a, long long idx) {
    const float v = a.in[idx];
    return a.pm1 ? v * 0.5f + 0.5f : v;
}
__device__ __forceinline__ float aug_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ void aug_out(const AugArgs& a, long long idx, float v, bool clamp) {
    if (clamp || a.pm1) v = aug_clamp01(v);
    a.out[idx] = a.pm1 ? v * 2.0f - 1.0f : v;
}
// pixel (y, x) of the plane after `q` counter-clockwise quarter turns (torch.rot90 on the last two dims), read from the original plane
__device__ __forceinline__ float aug_rot90_px(const AugArgs& a, long long plane, int q, int y, int x) {
    const int H = a.H, W = a.W;
    int sy, sx;
    if (q == 0) { sy = y; sx = x; }
    else if (q == 1) { sy = x; sx = W - 1 - y; }
    else if (q == 2) { sy = H - 1 - y; sx = W - 1 - x; }
    else { sy = H - 1 - x; sx = y; }
    return aug_in(a, plane * H * W + (long long)sy * W + sx);
}

// 16 x 16 output pixels per workgroup, the (16 + k - 1)^2 reflect-padded patch in LDS
__global__ __launch_bounds__(256) void k_aug_blur(AugArgs a) {
    extern __shared__ float tile[];
    const int k = a.k, p = k / 2, TW = 16 + k - 1;
    const long long plane = blockIdx.z;
    const int y0 = blockIdx.y * 16, x0 = blockIdx.x * 16;
    for (int t = threadIdx.x; t < TW * TW; t += 256) {
        int yy = y0 + t / TW - p, xx = x0 + t % TW - p;
        yy = yy < 0 ? -yy : (yy >= a.H ? 2 * (a.H - 1) - yy : yy);
        xx = xx < 0 ? -xx : (xx >= a.W ? 2 * (a.W - 1) - xx : xx);
        yy = yy < 0 ? 0 : (yy >= a.H ? a.H - 1 : yy);          // tiles past the image edge (ragged sizes): any in-bounds pixel
        xx = xx < 0 ? 0 : (xx >= a.W ? a.W - 1 : xx);
        tile[t] = aug_in(a, plane * a.H * a.W + (long long)yy * a.W + xx);
    }
    __syncthreads();
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= a.H || x >= a.W) return;
    float acc = 0.f;
    for (int i = 0; i < k; ++i) {
        const float wi = a.w[i];
        for (int j = 0; j < k; ++j) acc = fmaf(wi * a.w[j], tile[(ty + i) * TW + tx + j], acc);
    }
    aug_out(a, plane * a.H * a.W + (long long)y * a.W + x, acc, true);
}

template <int OP>
__global__ __launch_bounds__(256) void k_aug_point(AugArgs a) {
    const long long n = (long long)a.planes * a.H * a.W;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int x = (int)(idx % a.W), y = (int)((idx / a.W) % a.H);
    const long long plane = idx / ((long long)a.W * a.H);
    if (OP == AUG_IDENTITY) aug_out(a, idx, aug_in(a, idx), false);
    else if (OP == AUG_NOISE) aug_out(a, idx, aug_in(a, idx) + a.f * a.noise[idx], true);
    else if (OP == AUG_BRIGHTNESS) aug_out(a, idx, aug_in(a, idx) * a.f, true);
    else if (OP == AUG_FLIP_H) aug_out(a, idx, aug_in(a, plane * a.H * a.W + (long long)y * a.W + (a.W - 1 - x)), false);
    else if (OP == AUG_CROP_PAD) aug_out(a, idx, (y < a.nh && x < a.nw) ? aug_in(a, idx) : 0.f, false);
    else if (OP == AUG_ROTATE) {
        // the canvas after the quarter turns (square images keep their shape; the host rejects odd quarter turns of non-square ones)
        float v;
        if (!a.has_rest) v = aug_rot90_px(a, plane, a.quarters, y, x);
        else {
            const float dx = (float)x + 0.5f - 0.5f * (float)a.W, dy = (float)y + 0.5f - 0.5f * (float)a.H;
            const float sx = a.cs * dx - a.sn * dy, sy = a.sn * dx + a.cs * dy;          // inverse map of a counter-clockwise rotation
            const float fx = rintf(sx + 0.5f * (float)a.W - 0.5f), fy = rintf(sy + 0.5f * (float)a.H - 0.5f);
            v = (fx >= 0.f && fx < (float)a.W && fy >= 0.f && fy < (float)a.H) ? aug_rot90_px(a, plane, a.quarters, (int)fy, (int)fx) : 0.f;
        }
        aug_out(a, idx, v, false);
    } else if (OP == AUG_CROP_RESIZE) {
        // triangle filter of support max(scale, 1) around the source centre scale * (i + 0.5), weights normalised per axis
        const float scy = (float)a.nh / (float)a.H, scx = (float)a.nw / (float)a.W;
        const float spy = fmaxf(scy, 1.f), spx = fmaxf(scx, 1.f);
        const float cy = scy * ((float)y + 0.5f), cx = scx * ((float)x + 0.5f);
        const int ylo = max((int)(cy - spy + 0.5f), 0), yhi = min((int)(cy + spy + 0.5f), a.nh);
        const int xlo = max((int)(cx - spx + 0.5f), 0), xhi = min((int)(cx + spx + 0.5f), a.nw);
        float wys = 0.f, wxs = 0.f;
        for (int j = ylo; j < yhi; ++j) wys += fmaxf(0.f, 1.f - fabsf(((float)j - cy + 0.5f) / spy));
        for (int j = xlo; j < xhi; ++j) wxs += fmaxf(0.f, 1.f - fabsf(((float)j - cx + 0.5f) / spx));
        float acc = 0.f;
        for (int i = ylo; i < yhi; ++i) {
            const float wy = fmaxf(0.f, 1.f - fabsf(((float)i - cy + 0.5f) / spy)) / wys;
            float row = 0.f;
            for (int j = xlo; j < xhi; ++j) {
                const float wx = fmaxf(0.f, 1.f - fabsf(((float)j - cx + 0.5f) / spx)) / wxs;
                row = fmaf(wx, aug_in(a, plane * a.H * a.W + (long long)i * a.W + j), row);
            }
            acc = fmaf(wy, row, acc);
        }
        aug_out(a, idx, acc, false);
    }
}

}  // namespace wmar

using namespace wmar;

extern "C" int wmar_augment(int32_t op, const float* in_dev, float* out_dev, const float* noise_dev, int64_t B, int32_t C, int32_t H,
                            int32_t W, int32_t pm1, double p0, double p1, void* stream) {
    WMAR_REQUIRE(in_dev && out_dev && B >= 1 && C >= 1 && H >= 1 && W >= 1, "augment: bad argument");
    WMAR_REQUIRE(in_dev != out_dev || op == AUG_NOISE || op == AUG_BRIGHTNESS || op == AUG_IDENTITY, "augment: this transform cannot run in place");
    AugArgs a{};
    a.in = in_dev; a.out = out_dev; a.noise = noise_dev; a.planes = (int)(B * C); a.H = H; a.W = W; a.pm1 = pm1 ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)a.planes * H * W;
    const dim3 pgrid((unsigned)((n + 255) / 256));
    switch (op) {
        case AUG_IDENTITY: hipLaunchKernelGGL(k_aug_point<AUG_IDENTITY>, pgrid, dim3(256), 0, st, a); break;
        case AUG_BLUR: {
            const int k = (int)p0;
            WMAR_REQUIRE(k >= 1 && k <= AUG_MAX_K && (k & 1), "augment: blur kernel size %d (odd, 1..%d)", k, AUG_MAX_K);
            WMAR_REQUIRE(k / 2 < H && k / 2 < W, "augment: blur kernel %d does not fit a %d x %d image (reflect padding)", k, H, W);
            WMAR_REQUIRE(B * C <= 65535, "augment: blur of %lld planes (the launch takes at most 65535)", (long long)(B * C));      // planes are gridDim.z
            // gaussian_blur's weights: x = -(k-1)/2 .. (k-1)/2, exp(-x^2 / 2 sigma^2), normalised (float, as torchvision computes them in the image dtype)
            const float sigma = 0.3f * ((float)(k - 1) * 0.5f - 1.f) + 0.8f;
            float sum = 0.f;
            for (int i = 0; i < k; ++i) {
                const float x = -(float)(k - 1) * 0.5f + (float)i;
                a.w[i] = expf(-0.5f * (x / sigma) * (x / sigma));
                sum += a.w[i];
            }
            for (int i = 0; i < k; ++i) a.w[i] /= sum;
            a.k = k;
            const int TW = 16 + k - 1;
            hipLaunchKernelGGL(k_aug_blur, dim3((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16), (unsigned)a.planes), dim3(256),
                               (size_t)TW * TW * sizeof(float), st, a);
            break;
        }
        case AUG_NOISE:
            WMAR_REQUIRE(noise_dev, "augment: the noise transform needs its standard normal draws");
            a.f = (float)p0;
            hipLaunchKernelGGL(k_aug_point<AUG_NOISE>, pgrid, dim3(256), 0, st, a);
            break;
        case AUG_BRIGHTNESS:
            a.f = (float)p0;
            hipLaunchKernelGGL(k_aug_point<AUG_BRIGHTNESS>, pgrid, dim3(256), 0, st, a);
            break;
        case AUG_ROTATE: {
            // p0: counter-clockwise quarter turns (0..3), p1: remainder angle in degrees, [0, 90)
            a.quarters = ((int)p0 % 4 + 4) % 4;
            WMAR_REQUIRE(H == W || a.quarters % 2 == 0, "augment: odd quarter turns need a square image");
            const double rad = p1 * 3.14159265358979323846 / 180.0;
            a.has_rest = p1 != 0.0 ? 1 : 0;
            a.cs = (float)cos(rad); a.sn = (float)sin(rad);
            hipLaunchKernelGGL(k_aug_point<AUG_ROTATE>, pgrid, dim3(256), 0, st, a);
            break;
        }
        case AUG_FLIP_H: hipLaunchKernelGGL(k_aug_point<AUG_FLIP_H>, pgrid, dim3(256), 0, st, a); break;
        case AUG_CROP_RESIZE:
        case AUG_CROP_PAD:
            a.nh = (int)p0; a.nw = (int)p1;
            WMAR_REQUIRE(a.nh >= 1 && a.nh <= H && a.nw >= 1 && a.nw <= W, "augment: crop %d x %d of a %d x %d image", a.nh, a.nw, H, W);
            if (op == AUG_CROP_RESIZE) hipLaunchKernelGGL(k_aug_point<AUG_CROP_RESIZE>, pgrid, dim3(256), 0, st, a);
            else hipLaunchKernelGGL(k_aug_point<AUG_CROP_PAD>, pgrid, dim3(256), 0, st, a);
            break;
        default: set_error("augment: unknown transform %d", op); return WMAR_EINVAL;
    }
    return launch_status("k_aug");
}

// ---------------------------------------------------------------------------------------------------------------- backward
// The vector-Jacobian product of every transform above, as the forward is implemented (range change and clamp included), for training
// through the transforms (finetune.py: decode, augment, re-encode, MSE on the latents; wmar/utils/utils.py:25-44).  With T the
// transform in [0, 1]: out = 2 clamp(T(x / 2 + 0.5)) - 1 in `pm1` mode, so grad_x = 0.5 T^T(2 g mask); the factors are exact.  The
// mask is 0 <= t <= 1 INCLUSIVE (torch's clamp passes the gradient at both bounds), with t recomputed by the forward's own expression,
// so it agrees bit for bit with what the forward clipped.  Every kernel is in gather form -- one thread owns one grad_in element and
// adds its contributions in a fixed order -- so there are no atomics and two runs give the same bits.
namespace wmar {

struct AugBwdArgs {
    AugArgs a;              // the forward's arguments (a.out is not used)
    const float* g;         // gradient with respect to the forward's output
    float* gin;             // gradient with respect to the forward's input
    float* ws;              // blur: g * mask between the two launches
};

// the gradient that enters T^T at an output pixel whose value before the clamp was `t`
__device__ __forceinline__ float aug_gmask(const AugArgs& a, float g, float t, bool clamp) {
    if ((clamp || a.pm1) && !(t >= 0.f && t <= 1.f)) return 0.f;
    return a.pm1 ? g * 2.0f : g;
}
__device__ __forceinline__ float aug_gin(const AugArgs& a, float v) { return a.pm1 ? v * 0.5f : v; }

// crop + resize: window [lo, hi), centre and weight sum of output coordinate `o` along an axis with `n` kept pixels (the forward's expressions)
__device__ __forceinline__ void aug_resize_win(float sc, float sp, int o, int n, int& lo, int& hi, float& c, float& wsum) {
    c = sc * ((float)o + 0.5f);
    lo = max((int)(c - sp + 0.5f), 0);
    hi = min((int)(c + sp + 0.5f), n);
    wsum = 0.f;
    for (int j = lo; j < hi; ++j) wsum += fmaxf(0.f, 1.f - fabsf(((float)j - c + 0.5f) / sp));
}
// crop + resize: the forward's value at output pixel (y, x) before the clamp, same operations in the same order
__device__ __forceinline__ float aug_resize_t(const AugArgs& a, long long plane, int y, int x) {
    const float scy = (float)a.nh / (float)a.H, scx = (float)a.nw / (float)a.W;
    const float spy = fmaxf(scy, 1.f), spx = fmaxf(scx, 1.f);
    int ylo, yhi, xlo, xhi;
    float cy, cx, wys, wxs;
    aug_resize_win(scy, spy, y, a.nh, ylo, yhi, cy, wys);
    aug_resize_win(scx, spx, x, a.nw, xlo, xhi, cx, wxs);
    float acc = 0.f;
    for (int i = ylo; i < yhi; ++i) {
        const float wy = fmaxf(0.f, 1.f - fabsf(((float)i - cy + 0.5f) / spy)) / wys;
        float row = 0.f;
        for (int j = xlo; j < xhi; ++j) {
            const float wx = fmaxf(0.f, 1.f - fabsf(((float)j - cx + 0.5f) / spx)) / wxs;
            row = fmaf(wx, aug_in(a, plane * a.H * a.W + (long long)i * a.W + j), row);
        }
        acc = fmaf(wy, row, acc);
    }
    return acc;
}
// crop + resize: first and last output coordinate whose window can contain source pixel `s` (a superset; the window test decides)
__device__ __forceinline__ void aug_resize_span(float sc, float sp, int s, int n_out, int& first, int& last) {
    const float lo = floorf(((float)s - sp - 1.f) / sc) - 1.f, hi = ceilf(((float)s + sp + 2.f) / sc) + 1.f;
    first = (int)fmaxf(lo, 0.f);
    last = (int)fminf(hi, (float)(n_out - 1));
}

// One thread per INPUT pixel (y, x) of plane `plane`.
template <int OP>
__global__ __launch_bounds__(256) void k_aug_bwd_point(AugBwdArgs b) {
    const AugArgs& a = b.a;
    const long long n = (long long)a.planes * a.H * a.W;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int x = (int)(idx % a.W), y = (int)((idx / a.W) % a.H);
    const long long plane = idx / ((long long)a.W * a.H), base = plane * a.H * a.W;
    if (OP == AUG_IDENTITY) b.gin[idx] = aug_gin(a, aug_gmask(a, b.g[idx], aug_in(a, idx), false));
    else if (OP == AUG_NOISE) b.gin[idx] = aug_gin(a, aug_gmask(a, b.g[idx], aug_in(a, idx) + a.f * a.noise[idx], true));
    else if (OP == AUG_BRIGHTNESS) b.gin[idx] = aug_gin(a, aug_gmask(a, b.g[idx], aug_in(a, idx) * a.f, true) * a.f);
    else if (OP == AUG_FLIP_H) b.gin[idx] = aug_gin(a, aug_gmask(a, b.g[base + (long long)y * a.W + (a.W - 1 - x)], aug_in(a, idx), false));
    else if (OP == AUG_CROP_PAD) b.gin[idx] = (y < a.nh && x < a.nw) ? aug_gin(a, aug_gmask(a, b.g[idx], aug_in(a, idx), false)) : 0.f;
    else if (OP == AUG_ROTATE) {
        // (cy, cx): this pixel on the canvas after the quarter turns -- aug_rot90_px inverted
        const int H = a.H, W = a.W, q = a.quarters;
        int cy, cx;
        if (q == 0) { cy = y; cx = x; }
        else if (q == 1) { cy = W - 1 - x; cx = y; }
        else if (q == 2) { cy = H - 1 - y; cx = W - 1 - x; }
        else { cy = x; cx = H - 1 - y; }
        const float t = aug_in(a, idx);         // every output that reads this pixel has this value before the clamp
        float acc = 0.f;
        if (!a.has_rest) acc = aug_gmask(a, b.g[base + (long long)cy * W + cx], t, false);
        else {
            // nearest sampling is no bijection: forward-map the centre, then keep the outputs of the 3 x 3 neighbourhood whose source
            // coordinates (the forward's own float expression) land on this pixel, in raster order
            const float ux = (float)cx + 0.5f - 0.5f * (float)W, uy = (float)cy + 0.5f - 0.5f * (float)H;
            const int ox0 = (int)rintf(a.cs * ux + a.sn * uy + 0.5f * (float)W - 0.5f);
            const int oy0 = (int)rintf(a.cs * uy - a.sn * ux + 0.5f * (float)H - 0.5f);
            for (int oy = max(oy0 - 1, 0); oy <= min(oy0 + 1, H - 1); ++oy)
                for (int ox = max(ox0 - 1, 0); ox <= min(ox0 + 1, W - 1); ++ox) {
                    const float dx = (float)ox + 0.5f - 0.5f * (float)W, dy = (float)oy + 0.5f - 0.5f * (float)H;
                    const float sx = a.cs * dx - a.sn * dy, sy = a.sn * dx + a.cs * dy;
                    const float fx = rintf(sx + 0.5f * (float)W - 0.5f), fy = rintf(sy + 0.5f * (float)H - 0.5f);
                    if (fx == (float)cx && fy == (float)cy) acc += aug_gmask(a, b.g[base + (long long)oy * W + ox], t, false);
                }
        }
        b.gin[idx] = aug_gin(a, acc);
    } else if (OP == AUG_CROP_RESIZE) {
        // transpose of the separable triangle filter: the outputs whose windows contain this pixel, weights recomputed and normalised
        // as the forward does; pixels outside the crop are never read
        float acc = 0.f;
        if (y < a.nh && x < a.nw) {
            const float scy = (float)a.nh / (float)a.H, scx = (float)a.nw / (float)a.W;
            const float spy = fmaxf(scy, 1.f), spx = fmaxf(scx, 1.f);
            int oya, oyb, oxa, oxb;
            aug_resize_span(scy, spy, y, a.H, oya, oyb);
            aug_resize_span(scx, spx, x, a.W, oxa, oxb);
            for (int oy = oya; oy <= oyb; ++oy) {
                int lo, hi;
                float c, wsum;
                aug_resize_win(scy, spy, oy, a.nh, lo, hi, c, wsum);
                if (y < lo || y >= hi) continue;
                const float wy = fmaxf(0.f, 1.f - fabsf(((float)y - c + 0.5f) / spy)) / wsum;
                float row = 0.f;
                for (int ox = oxa; ox <= oxb; ++ox) {
                    aug_resize_win(scx, spx, ox, a.nw, lo, hi, c, wsum);
                    if (x < lo || x >= hi) continue;
                    const float wx = fmaxf(0.f, 1.f - fabsf(((float)x - c + 0.5f) / spx)) / wsum;
                    const float t = a.pm1 ? aug_resize_t(a, plane, oy, ox) : 0.f;           // no clamp without pm1
                    row = fmaf(wx, aug_gmask(a, b.g[base + (long long)oy * a.W + ox], t, false), row);
                }
                acc = fmaf(wy, row, acc);
            }
        }
        b.gin[idx] = aug_gin(a, acc);
    }
}

// Blur, launch 1: recompute the forward's t (k_aug_blur's tile scheme and summation order) and write m = g * mask to the workspace
__global__ __launch_bounds__(256) void k_aug_bwd_blur_mask(AugBwdArgs b) {
    extern __shared__ float tile[];
    const AugArgs& a = b.a;
    const int k = a.k, p = k / 2, TW = 16 + k - 1;
    const long long plane = blockIdx.z;
    const int y0 = blockIdx.y * 16, x0 = blockIdx.x * 16;
    for (int t = threadIdx.x; t < TW * TW; t += 256) {
        int yy = y0 + t / TW - p, xx = x0 + t % TW - p;
        yy = yy < 0 ? -yy : (yy >= a.H ? 2 * (a.H - 1) - yy : yy);
        xx = xx < 0 ? -xx : (xx >= a.W ? 2 * (a.W - 1) - xx : xx);
        yy = yy < 0 ? 0 : (yy >= a.H ? a.H - 1 : yy);
        xx = xx < 0 ? 0 : (xx >= a.W ? a.W - 1 : xx);
        tile[t] = aug_in(a, plane * a.H * a.W + (long long)yy * a.W + xx);
    }
    __syncthreads();
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= a.H || x >= a.W) return;
    float acc = 0.f;
    for (int i = 0; i < k; ++i) {
        const float wi = a.w[i];
        for (int j = 0; j < k; ++j) acc = fmaf(wi * a.w[j], tile[(ty + i) * TW + tx + j], acc);
    }
    const long long o = plane * a.H * a.W + (long long)y * a.W + x;
    b.ws[o] = aug_gmask(a, b.g[o], acc, true);
}

// Blur: what source `s` receives from output `o` along an axis of `n` pixels.  The forward reads the reflect-padded axis, so s stands
// at the padded positions q = s, -s (1 <= s <= p) and 2 (n - 1) - s (s <= n - 2, within p of the far edge); output o reads position
// q with tap q - o + p.  `w` are the forward's weights (LDS).
__device__ __forceinline__ float aug_blur_adjoint_w(const float* w, int k, int s, int o, int n) {
    const int p = k / 2;
    float r = 0.f;
    int i = s - o + p;
    if (i >= 0 && i < k) r += w[i];
    if (s >= 1 && s <= p) {
        i = -s - o + p;
        if (i >= 0 && i < k) r += w[i];
    }
    if (s <= n - 2 && n - 1 - s <= p) {
        i = 2 * (n - 1) - s - o + p;
        if (i >= 0 && i < k) r += w[i];
    }
    return r;
}

// Blur, launch 2: the adjoint of the reflect-padded separable correlation applied to m.  16 x 16 sources per workgroup; every output
// that reads source s lies within p of it, so the (16 + k - 1)^2 patch of m (zero outside the image) is all a workgroup needs.  Rows
// first, then columns, each a k-term sum in tap order.
__global__ __launch_bounds__(256) void k_aug_bwd_blur(AugBwdArgs b) {
    extern __shared__ float tile[];
    const AugArgs& a = b.a;
    const int k = a.k, p = k / 2, TW = 16 + k - 1;
    float* hsum = tile + TW * TW;               // [TW][16] row sums
    float* wye = hsum + TW * 16;                // [16][k] adjoint weights of the tile's rows
    float* wxe = wye + 16 * k;                  // [16][k] ... and columns
    float* wl = wxe + 16 * k;                   // [k] the forward's weights
    const long long plane = blockIdx.z;
    const int y0 = blockIdx.y * 16, x0 = blockIdx.x * 16;
    for (int t = threadIdx.x; t < k; t += 256) wl[t] = a.w[t];
    for (int t = threadIdx.x; t < TW * TW; t += 256) {
        const int yy = y0 + t / TW - p, xx = x0 + t % TW - p;
        tile[t] = (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) ? b.ws[plane * a.H * a.W + (long long)yy * a.W + xx] : 0.f;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 16 * k; t += 256) {
        const int s = t / k, j = t % k;
        wye[t] = aug_blur_adjoint_w(wl, k, y0 + s, y0 + s - p + j, a.H);
        wxe[t] = aug_blur_adjoint_w(wl, k, x0 + s, x0 + s - p + j, a.W);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < TW * 16; t += 256) {
        const int r = t / 16, c = t % 16;
        float acc = 0.f;
        for (int j = 0; j < k; ++j) acc = fmaf(wxe[c * k + j], tile[r * TW + c + j], acc);
        hsum[t] = acc;
    }
    __syncthreads();
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= a.H || x >= a.W) return;
    float acc = 0.f;
    for (int i = 0; i < k; ++i) acc = fmaf(wye[ty * k + i], hsum[(ty + i) * 16 + tx], acc);
    b.gin[plane * a.H * a.W + (long long)y * a.W + x] = aug_gin(a, acc);
}

// gaussian_blur's weights exactly as wmar_augment computes them (float, in the image dtype).  A COPY of the lines in wmar_augment's blur
// case, which stays as it was: the two must remain identical operation for operation -- launch 1 recomputes the forward's t with these
// weights, and the mask agrees with what the forward clipped only while they are the same bits.
static void aug_blur_weights(int k, float* w) {
    const float sigma = 0.3f * ((float)(k - 1) * 0.5f - 1.f) + 0.8f;
    float sum = 0.f;
    for (int i = 0; i < k; ++i) {
        const float x = -(float)(k - 1) * 0.5f + (float)i;
        w[i] = expf(-0.5f * (x / sigma) * (x / sigma));
        sum += w[i];
    }
    for (int i = 0; i < k; ++i) w[i] /= sum;
}

}  // namespace wmar

extern "C" int wmar_augment_backward(int32_t op, const float* in_dev, const float* grad_out_dev, float* grad_in_dev, const float* noise_dev,
                                     float* workspace_dev, int64_t B, int32_t C, int32_t H, int32_t W, int32_t pm1, double p0, double p1,
                                     void* stream) {
    // every check before any launch
    WMAR_REQUIRE(in_dev && grad_out_dev && grad_in_dev && B >= 1 && C >= 1 && H >= 1 && W >= 1 && B * C <= 0x7fffffff,
                 "augment_backward: bad argument");
    WMAR_REQUIRE(op >= AUG_IDENTITY && op <= AUG_CROP_PAD, "augment_backward: unknown transform %d", op);
    // a thread of these four reads grad_out at its own element only; every other transform gathers from its neighbours
    const bool own_element = op == AUG_IDENTITY || op == AUG_NOISE || op == AUG_BRIGHTNESS || op == AUG_CROP_PAD;
    WMAR_REQUIRE(own_element || (grad_in_dev != grad_out_dev && grad_in_dev != in_dev),
                 "augment_backward: the gradient of this transform cannot be written in place");
    AugBwdArgs b{};
    AugArgs& a = b.a;
    a.in = in_dev; a.noise = noise_dev; a.planes = (int)(B * C); a.H = H; a.W = W; a.pm1 = pm1 ? 1 : 0;
    b.g = grad_out_dev; b.gin = grad_in_dev; b.ws = workspace_dev;
    switch (op) {
        case AUG_BLUR: {
            const int k = (int)p0;
            WMAR_REQUIRE(k >= 1 && k <= AUG_MAX_K && (k & 1), "augment_backward: blur kernel size %d (odd, 1..%d)", k, AUG_MAX_K);
            WMAR_REQUIRE(k / 2 < H && k / 2 < W, "augment_backward: blur kernel %d does not fit a %d x %d image (reflect padding)", k, H, W);
            WMAR_REQUIRE(B * C <= 65535, "augment_backward: blur of %lld planes (the launches take at most 65535)", (long long)(B * C));
            WMAR_REQUIRE(workspace_dev, "augment_backward: blur needs a workspace of B * C * H * W floats");
            WMAR_REQUIRE(workspace_dev != grad_in_dev && workspace_dev != grad_out_dev && workspace_dev != in_dev,
                         "augment_backward: the workspace overlaps another buffer");
            aug_blur_weights(k, a.w);
            a.k = k;
            break;
        }
        case AUG_NOISE:
            WMAR_REQUIRE(noise_dev, "augment_backward: the noise transform needs its standard normal draws");
            a.f = (float)p0;
            break;
        case AUG_BRIGHTNESS: a.f = (float)p0; break;
        case AUG_ROTATE: {
            a.quarters = ((int)p0 % 4 + 4) % 4;
            WMAR_REQUIRE(H == W || a.quarters % 2 == 0, "augment_backward: odd quarter turns need a square image");
            const double rad = p1 * 3.14159265358979323846 / 180.0;
            a.has_rest = p1 != 0.0 ? 1 : 0;
            a.cs = (float)cos(rad); a.sn = (float)sin(rad);
            break;
        }
        case AUG_CROP_RESIZE:
        case AUG_CROP_PAD:
            a.nh = (int)p0; a.nw = (int)p1;
            WMAR_REQUIRE(a.nh >= 1 && a.nh <= H && a.nw >= 1 && a.nw <= W, "augment_backward: crop %d x %d of a %d x %d image", a.nh, a.nw, H, W);
            break;
        default: break;
    }
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)a.planes * H * W;
    const dim3 pgrid((unsigned)((n + 255) / 256));
    switch (op) {
        case AUG_IDENTITY: hipLaunchKernelGGL(k_aug_bwd_point<AUG_IDENTITY>, pgrid, dim3(256), 0, st, b); break;
        case AUG_BLUR: {
            const int k = a.k, TW = 16 + k - 1;
            const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16), (unsigned)a.planes);
            hipLaunchKernelGGL(k_aug_bwd_blur_mask, grid, dim3(256), (size_t)TW * TW * sizeof(float), st, b);
            hipLaunchKernelGGL(k_aug_bwd_blur, grid, dim3(256), (size_t)(TW * TW + TW * 16 + 33 * k) * sizeof(float), st, b);
            break;
        }
        case AUG_NOISE: hipLaunchKernelGGL(k_aug_bwd_point<AUG_NOISE>, pgrid, dim3(256), 0, st, b); break;
        case AUG_BRIGHTNESS: hipLaunchKernelGGL(k_aug_bwd_point<AUG_BRIGHTNESS>, pgrid, dim3(256), 0, st, b); break;
        case AUG_ROTATE: hipLaunchKernelGGL(k_aug_bwd_point<AUG_ROTATE>, pgrid, dim3(256), 0, st, b); break;
        case AUG_FLIP_H: hipLaunchKernelGGL(k_aug_bwd_point<AUG_FLIP_H>, pgrid, dim3(256), 0, st, b); break;
        case AUG_CROP_RESIZE: hipLaunchKernelGGL(k_aug_bwd_point<AUG_CROP_RESIZE>, pgrid, dim3(256), 0, st, b); break;
        default: hipLaunchKernelGGL(k_aug_bwd_point<AUG_CROP_PAD>, pgrid, dim3(256), 0, st, b); break;
    }
    return launch_status("k_aug_bwd");
}
