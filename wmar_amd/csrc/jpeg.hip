// JPEG round trip of the evaluation sweep (AugmentationManager "jpeg", generate.py:142-164) on the device, bit for bit what PIL's
// save(format="JPEG", quality=q) + Image.open(...).convert("RGB") returns (libjpeg-turbo's default baseline path).  Entropy coding is
// lossless, so the decoded pixels are an integer function of the input pixels and q; no bitstream is written.
//
// Reference: wmar/augmentations/valuemetric.py:30-75 (ToPILImage -> PIL JPEG -> ToTensor per image).  libjpeg-turbo steps restated
// (tests/jpeg_reference.py holds the same steps in numpy, pinned to PIL by tests/test_jpeg_integer_pipeline.py):
//   jccolor.c rgb_ycc_convert        RGB -> YCbCr, 16-bit fixed point
//   jcsample.c h2v2_downsample       2 x 2 box sums of Cb / Cr, bias 1, 2, 1, 2, ... along each output row
//   jfdctint.c jpeg_fdct_islow       on sample - 128, rows then columns
//   jcdctmgr.c quantize              by 8 t, half away from zero; t = Annex K tables scaled as jpeg_set_quality(q, TRUE)
//   jidctint.c jpeg_idct_islow       on k t, columns then rows, post-IDCT range-limit table (index & 1023)
//   jdsample.c h2v2_fancy_upsample   triangle filter, first / last chroma row and column replicated
//   jdcolor.c ycc_rgb_convert        YCbCr -> RGB, 16-bit fixed point, clamped to [0, 255]
// Entry and exit are the module's float steps: u = (uint8)(clamp(x, 0, 1) * 255), c = u / 255 (correctly rounded, a compile-time
// table), passthrough output x + (c - x) in fp32, clamp; with pm1 the [-1, 1] <-> [0, 1] range changes of the harness around it.
//
// Two launches per (batch, quality), H and W multiples of 16:
//   k_jpeg_code  one 64-lane workgroup per 16 x 16 MCU (four Y blocks, one Cb, one Cr): colour conversion, downsampling, forward DCT,
//                quantisation, dequantisation, inverse DCT; the reconstructed Y / Cb / Cr samples go to the caller's workspace
//                (1.5 bytes per pixel)
//   k_jpeg_out   one thread per 4 pixels of a row: fancy upsampling of the reconstructed chroma (needs the neighbouring MCUs'
//                samples, hence the second launch), YCbCr -> RGB, exit.
#include "common.h"

namespace wmar {

// ITU T.81 Annex K tables, natural order (jcparam.c std_luminance_quant_tbl / std_chrominance_quant_tbl)
__constant__ int jpeg_std_tables[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
     103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// u / 255.0f for u = 0..255, folded by the compiler (IEEE division, round to nearest even): ToTensor's division, exactly
struct JpegUnitTable {
    float v[256];
    constexpr JpegUnitTable() : v() {
        for (int i = 0; i < 256; ++i) v[i] = (float)i / 255.0f;
    }
};
__constant__ JpegUnitTable jpeg_unit = JpegUnitTable();

struct JpegArgs {
    const float* in;
    float* out;
    uint8_t* ws;            // reconstructed samples: Y [B][H][W], then Cb [B][H/2][W/2], then Cr [B][H/2][W/2]
    long long n;            // k_jpeg_code: MCUs (B * H/16 * W/16); k_jpeg_out: 4-pixel groups (B * H * W / 4)
    int H, W;
    int scale;              // jpeg_quality_scaling(q)
    int pm1, passthrough;
};

// fixed-point constants of jccolor.c / jdcolor.c: FIX(x) = (int)(x * 65536 + 0.5)
constexpr int JFIX(double x) { return (int)(x * 65536.0 + 0.5); }
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633;
constexpr int F1501 = 12299, F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;

__device__ __forceinline__ int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

__device__ __forceinline__ float jpeg_entry(float v, int pm1) {
    if (pm1) v = v * 0.5f + 0.5f;
    return fminf(fmaxf(v, 0.f), 1.f);
}

// one pass of jpeg_fdct_islow over 8 samples (FIRST: the row pass)
template <bool FIRST>
__device__ __forceinline__ void jpeg_fdct8(int* d) {
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int SH = FIRST ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
    if (FIRST) {
        d[0] = (tmp10 + tmp11) * (1 << PASS1_BITS);
        d[4] = (tmp10 - tmp11) * (1 << PASS1_BITS);
    } else {
        d[0] = jpeg_descale(tmp10 + tmp11, PASS1_BITS);
        d[4] = jpeg_descale(tmp10 - tmp11, PASS1_BITS);
    }
    const int z1e = (tmp12 + tmp13) * F0541;
    d[2] = jpeg_descale(z1e + tmp13 * F0765, SH);
    d[6] = jpeg_descale(z1e - tmp12 * F1847, SH);
    const int z5 = (tmp4 + tmp6 + tmp5 + tmp7) * F1175;
    const int z1 = (tmp4 + tmp7) * -F0899, z2 = (tmp5 + tmp6) * -F2562;
    const int z3 = (tmp4 + tmp6) * -F1961 + z5, z4 = (tmp5 + tmp7) * -F0390 + z5;
    d[7] = jpeg_descale(tmp4 * F0298 + z1 + z3, SH);
    d[5] = jpeg_descale(tmp5 * F2053 + z2 + z4, SH);
    d[3] = jpeg_descale(tmp6 * F3072 + z2 + z3, SH);
    d[1] = jpeg_descale(tmp7 * F1501 + z1 + z4, SH);
}

// one pass of jpeg_idct_islow over 8 values (FIRST: the column pass; the row pass leaves range-limit indices)
template <bool FIRST>
__device__ __forceinline__ void jpeg_idct8(int* d) {
    const int z1e = (d[2] + d[6]) * F0541;
    const int tmp2e = z1e - d[6] * F1847, tmp3e = z1e + d[2] * F0765;
    const int tmp0e = (d[0] + d[4]) * (1 << CONST_BITS), tmp1e = (d[0] - d[4]) * (1 << CONST_BITS);
    const int tmp10 = tmp0e + tmp3e, tmp13 = tmp0e - tmp3e, tmp11 = tmp1e + tmp2e, tmp12 = tmp1e - tmp2e;
    const int t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
    const int z5 = (t0 + t2 + t1 + t3) * F1175;
    const int z1 = (t0 + t3) * -F0899, z2 = (t1 + t2) * -F2562;
    const int z3 = (t0 + t2) * -F1961 + z5, z4 = (t1 + t3) * -F0390 + z5;
    const int tmp0 = t0 * F0298 + z1 + z3, tmp1 = t1 * F2053 + z2 + z4;
    const int tmp2 = t2 * F3072 + z2 + z3, tmp3 = t3 * F1501 + z1 + z4;
    constexpr int SH = FIRST ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS + 3;
    d[0] = jpeg_descale(tmp10 + tmp3, SH);
    d[7] = jpeg_descale(tmp10 - tmp3, SH);
    d[1] = jpeg_descale(tmp11 + tmp2, SH);
    d[6] = jpeg_descale(tmp11 - tmp2, SH);
    d[2] = jpeg_descale(tmp12 + tmp1, SH);
    d[5] = jpeg_descale(tmp12 - tmp1, SH);
    d[3] = jpeg_descale(tmp13 + tmp0, SH);
    d[4] = jpeg_descale(tmp13 - tmp0, SH);
}

// the decoder's post-IDCT range-limit table (jdmaster.c prepare_range_limit_table, offset by CENTERJSAMPLE)
__device__ __forceinline__ int jpeg_range_limit(int x) {
    const int v = x & 1023;
    return v < 128 ? v + 128 : (v < 512 ? 255 : (v < 896 ? 0 : v - 896));
}

__global__ __launch_bounds__(64) void k_jpeg_code(JpegArgs a) {
    __shared__ int cpx[2][16][16];      // full-resolution Cb, Cr of the MCU
    __shared__ int blk[6][64];          // 4 Y blocks (row-major 2 x 2), Cb, Cr; coefficients in place
    const long long m = blockIdx.x;
    if (m >= a.n) return;
    const int l = threadIdx.x;
    const int mw = a.W / 16, mh = a.H / 16;
    const long long b = m / ((long long)mw * mh);
    const int my = (int)((m / mw) % mh), mx = (int)(m % mw);
    const int y0 = my * 16, x0 = mx * 16;
    const long long HW = (long long)a.H * a.W;

    // colour conversion: lane -> 4 pixels of one MCU row
    {
        const int r = l >> 2, c0 = (l & 3) * 4;
        int u[3][4];
        for (int ch = 0; ch < 3; ++ch) {
            const float4 v = *reinterpret_cast<const float4*>(a.in + (b * 3 + ch) * HW + (long long)(y0 + r) * a.W + x0 + c0);
            u[ch][0] = (int)(jpeg_entry(v.x, a.pm1) * 255.0f);
            u[ch][1] = (int)(jpeg_entry(v.y, a.pm1) * 255.0f);
            u[ch][2] = (int)(jpeg_entry(v.z, a.pm1) * 255.0f);
            u[ch][3] = (int)(jpeg_entry(v.w, a.pm1) * 255.0f);
        }
        const int k = (r >> 3) * 2 + (c0 >> 3);
        for (int j = 0; j < 4; ++j) {
            const int R = u[0][j], G = u[1][j], B = u[2][j];
            const int Y = (JFIX(0.299) * R + JFIX(0.587) * G + JFIX(0.114) * B + (1 << 15)) >> 16;
            blk[k][(r & 7) * 8 + (c0 & 7) + j] = Y - 128;
            cpx[0][r][c0 + j] = (-JFIX(0.16874) * R - JFIX(0.33126) * G + JFIX(0.5) * B + (128 << 16) + (1 << 15) - 1) >> 16;
            cpx[1][r][c0 + j] = (JFIX(0.5) * R - JFIX(0.41869) * G - JFIX(0.08131) * B + (128 << 16) + (1 << 15) - 1) >> 16;
        }
    }
    __syncthreads();
    // h2v2 downsampling: lane -> one chroma sample of each plane; the MCU's chroma starts at an even column, so the bias is (1, 2)[cc & 1]
    {
        const int cr = l >> 3, cc = l & 7, bias = 1 + (cc & 1);
        for (int p = 0; p < 2; ++p) {
            const int s = cpx[p][2 * cr][2 * cc] + cpx[p][2 * cr][2 * cc + 1] + cpx[p][2 * cr + 1][2 * cc] + cpx[p][2 * cr + 1][2 * cc + 1];
            blk[4 + p][l] = ((s + bias) >> 2) - 128;
        }
    }
    __syncthreads();
    // lanes 0..47: (block, row) / (block, column) of the six 8 x 8 blocks
    const int k = l >> 3, i8 = l & 7;
    int d[8];
    if (l < 48) {                                               // forward DCT, rows
        for (int i = 0; i < 8; ++i) d[i] = blk[k][i8 * 8 + i];
        jpeg_fdct8<true>(d);
        for (int i = 0; i < 8; ++i) blk[k][i8 * 8 + i] = d[i];
    }
    __syncthreads();
    if (l < 48) {                                               // forward DCT, columns; quantise; dequantise; inverse DCT, columns
        for (int i = 0; i < 8; ++i) d[i] = blk[k][i * 8 + i8];
        jpeg_fdct8<false>(d);
        const int* base = jpeg_std_tables[k < 4 ? 0 : 1];
        for (int i = 0; i < 8; ++i) {
            const int t = min(max((base[i * 8 + i8] * a.scale + 50) / 100, 1), 255), dv = 8 * t;
            const int c = d[i], ac = abs(c) + (dv >> 1);
            const int q = ac >= dv ? ac / dv : 0;
            d[i] = (c < 0 ? -q : q) * t;
        }
        jpeg_idct8<true>(d);
        for (int i = 0; i < 8; ++i) blk[k][i * 8 + i8] = d[i];
    }
    __syncthreads();
    if (l < 48) {                                               // inverse DCT, rows; range limit; 8 samples to the workspace
        for (int i = 0; i < 8; ++i) d[i] = blk[k][i8 * 8 + i];
        jpeg_idct8<false>(d);
        unsigned lo = 0, hi = 0;
        for (int i = 0; i < 4; ++i) {
            lo |= (unsigned)jpeg_range_limit(d[i]) << (8 * i);
            hi |= (unsigned)jpeg_range_limit(d[4 + i]) << (8 * i);
        }
        uint8_t* dst;
        if (k < 4) {
            dst = a.ws + b * HW + (long long)(y0 + (k >> 1) * 8 + i8) * a.W + x0 + (k & 1) * 8;
        } else {
            const int Hc = a.H / 2, Wc = a.W / 2;
            const long long nb = a.n / ((long long)mw * mh);    // images in the batch
            dst = a.ws + nb * HW + (long long)(k - 4) * nb * Hc * Wc + b * Hc * Wc + (long long)(y0 / 2 + i8) * Wc + x0 / 2;
        }
        *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
    }
}

__global__ __launch_bounds__(256) void k_jpeg_out(JpegArgs a) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.n) return;
    const int W4 = a.W / 4, Hc = a.H / 2, Wc = a.W / 2;
    const int x0 = (int)(g % W4) * 4, y = (int)((g / W4) % a.H);
    const long long b = g / ((long long)W4 * a.H);
    const long long HW = (long long)a.H * a.W, nb = a.n / ((long long)W4 * a.H);
    const uchar4 yv = *reinterpret_cast<const uchar4*>(a.ws + b * HW + (long long)y * a.W + x0);
    const int Yv[4] = {yv.x, yv.y, yv.z, yv.w};
    // vertical step: 3 * nearer + further chroma row, edge rows replicated; columns cx - 1 .. cx + 2 around this group's cx, cx + 1
    const int cy = y >> 1, far = (y & 1) ? min(cy + 1, Hc - 1) : max(cy - 1, 0), cx = x0 >> 1;
    int up[2][4];
    for (int p = 0; p < 2; ++p) {
        const uint8_t* plane = a.ws + nb * HW + (long long)p * nb * Hc * Wc + b * Hc * Wc;
        int cs[4];
        for (int j = 0; j < 4; ++j) {
            const int c = min(max(cx - 1 + j, 0), Wc - 1);
            cs[j] = 3 * plane[(long long)cy * Wc + c] + plane[(long long)far * Wc + c];
        }
        // horizontal step; the first and last columns of the image use 4 * this
        up[p][0] = cx == 0 ? (4 * cs[1] + 8) >> 4 : (3 * cs[1] + cs[0] + 8) >> 4;
        up[p][1] = (3 * cs[1] + cs[2] + 7) >> 4;
        up[p][2] = (3 * cs[2] + cs[1] + 8) >> 4;
        up[p][3] = cx + 1 == Wc - 1 ? (4 * cs[2] + 7) >> 4 : (3 * cs[2] + cs[3] + 7) >> 4;
    }
    float c[3][4];
    for (int j = 0; j < 4; ++j) {
        const int cb = up[0][j] - 128, cr = up[1][j] - 128;
        const int R = Yv[j] + ((JFIX(1.402) * cr + (1 << 15)) >> 16);
        const int G = Yv[j] + ((-JFIX(0.71414) * cr - JFIX(0.34414) * cb + (1 << 15)) >> 16);
        const int B = Yv[j] + ((JFIX(1.772) * cb + (1 << 15)) >> 16);
        c[0][j] = jpeg_unit.v[min(max(R, 0), 255)];
        c[1][j] = jpeg_unit.v[min(max(G, 0), 255)];
        c[2][j] = jpeg_unit.v[min(max(B, 0), 255)];
    }
    for (int ch = 0; ch < 3; ++ch) {
        const long long off = (b * 3 + ch) * HW + (long long)y * a.W + x0;
        float o[4] = {c[ch][0], c[ch][1], c[ch][2], c[ch][3]};
        if (a.passthrough) {        // image + (coded - image), then the module's clamp
            const float4 v = *reinterpret_cast<const float4*>(a.in + off);
            const float xin[4] = {jpeg_entry(v.x, a.pm1), jpeg_entry(v.y, a.pm1), jpeg_entry(v.z, a.pm1), jpeg_entry(v.w, a.pm1)};
            for (int j = 0; j < 4; ++j) o[j] = fminf(fmaxf(xin[j] + (o[j] - xin[j]), 0.f), 1.f);
        }
        if (a.pm1)
            for (int j = 0; j < 4; ++j) o[j] = o[j] * 2.0f - 1.0f;
        *reinterpret_cast<float4*>(a.out + off) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

}  // namespace wmar

using namespace wmar;

extern "C" int64_t wmar_jpeg_workspace_bytes(int64_t B, int32_t H, int32_t W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    return B * H * W + 2 * B * (H / 2) * (W / 2);
}

extern "C" int wmar_jpeg(const float* in_dev, float* out_dev, void* workspace_dev, int64_t workspace_bytes, int64_t B, int32_t H,
                         int32_t W, int32_t quality, int32_t pm1, int32_t passthrough, void* stream) {
    WMAR_REQUIRE(in_dev && out_dev && B >= 1 && H >= 1 && W >= 1, "jpeg: bad argument");
    WMAR_REQUIRE(H % 16 == 0 && W % 16 == 0, "jpeg: %d x %d image (height and width must be multiples of 16)", H, W);
    WMAR_REQUIRE(quality >= 1 && quality <= 100, "jpeg: quality %d (1..100)", quality);
    WMAR_REQUIRE(in_dev != out_dev, "jpeg: cannot run in place");
    WMAR_REQUIRE(((uintptr_t)in_dev & 15) == 0 && ((uintptr_t)out_dev & 15) == 0 && ((uintptr_t)workspace_dev & 15) == 0,
                 "jpeg: buffers must be 16-byte aligned");
    const int64_t need = wmar_jpeg_workspace_bytes(B, H, W);
    WMAR_REQUIRE(workspace_dev && workspace_bytes >= need, "jpeg: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                 (long long)need);
    const long long mcus = (long long)B * (H / 16) * (W / 16), groups = (long long)B * H * W / 4;
    WMAR_REQUIRE((groups + 255) / 256 * 256 < (1LL << 32) && mcus * 64 < (1LL << 32), "jpeg: batch too large for one launch");
    JpegArgs a{};
    a.in = in_dev; a.out = out_dev; a.ws = (uint8_t*)workspace_dev; a.H = H; a.W = W;
    a.scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;          // jpeg_quality_scaling
    a.pm1 = pm1 ? 1 : 0; a.passthrough = passthrough ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    a.n = mcus;
    hipLaunchKernelGGL(k_jpeg_code, dim3((unsigned)mcus), dim3(64), 0, st, a);
    int rc = launch_status("k_jpeg_code");
    if (rc) return rc;
    a.n = groups;
    hipLaunchKernelGGL(k_jpeg_out, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, a);
    return launch_status("k_jpeg_out");
}
