// Image ingest on the device: what ImageTokenizer.img_tokens_from_pil does to a PIL image before the VQGAN sees it
// (deps/chameleon/inference/image_tokenizer.py:51-98: _whiten_transparency, then _vqgan_input_from = LANCZOS resize so that the short
// side equals the target, centre crop, u8 / 255 * 2 - 1), for a whole batch of images of any sizes, bit for bit what PIL returns.
//
// Pillow's 8-bit resample (src/libImaging/Resample.c) is integer arithmetic once its coefficient tables exist.  Steps restated
// (tests/lanczos_reference.py holds the same steps in numpy, pinned to PIL by tests/test_ingest_reference.py):
//   precompute_coeffs            per output pixel of one axis: the first input pixel, the number of taps and the LANCZOS weights
//                                (sinc(x) sinc(x / 3) on [-3, 3), stretched by max(in / out, 1)), normalised to sum 1, in double
//   normalize_coeffs_8bpc        weights to 22-bit fixed point, rounded half away from zero
//   ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc
//                                clip(((1 << 21) + sum pixel * weight) >> 22, 0, 255) in int32; the horizontal pass writes an 8-bit
//                                image and the vertical pass reads it: the rounding in between is part of the result
//   ImagingResample              an axis whose size does not change is not filtered
// The filter is an argument of the *_filtered entries (Pillow's numbers): BILINEAR swaps the weight function for the triangle 1 - |x|
// and the support 3 for 1 (what torchvision's Resize applies to a PIL image; precompute_codes.py) and shares every other step -- the
// kernels only see tables, and take any tap count from 1 up.
// The tables are built on the host in double (wmar_resample_coeffs, below) and uploaded; the kernels do the integer work.  The
// whitening (uint8)((1 - a / 255.0) * 255 + (a / 255.0) * c) in float64 is a 64 KB table built on the host, applied while the
// input row sits in LDS; the exit (float)((double)u / 255.0 * 2.0 - 1.0) is a compile-time table.
//
// Only what the crop window needs is computed: its T output columns and rows, and of the input only the rows the window's vertical
// taps touch and the columns its horizontal taps touch.  Two launches per batch, whatever the images' sizes (a descriptor per image
// on the device; the grids are sized for the largest image and blocks beyond an image's extent leave at once):
//   k_ingest_h   one workgroup per (64 output columns, 4 needed input rows, image): the rows' input segment is staged in LDS with
//                aligned dword loads, whitened there when the image is RGBA, and every thread filters one output pixel of one row;
//                uint8 intermediate [rows, T, 3]
//   k_ingest_v   one thread per output pixel (the T x T window flattened over 256-thread workgroups): filters the intermediate's column, writes the float CHW output and the cropped bytes
#include <cmath>
#include <mutex>
#include <tuple>

#include "common.h"

namespace wmar {

constexpr int INGEST_BITS = 22;                  // Pillow's PRECISION_BITS: 32 - 8 - 2
constexpr int INGEST_MAX_SIDE = 32768;
constexpr int INGEST_HC = 64, INGEST_HR = 4;     // k_ingest_h: output columns x input rows per workgroup
constexpr int INGEST_TILE = 2048;                // input pixels per row staged at once
constexpr int INGEST_ROW_BYTES = INGEST_TILE * 4 + 8;

struct IngestExitTable {
    float v[256];
    constexpr IngestExitTable() : v() {
        for (int i = 0; i < 256; ++i) v[i] = (float)((double)i / 255.0 * 2.0 - 1.0);
    }
};
__constant__ IngestExitTable ingest_exit = IngestExitTable();

// One image as the kernels see it.  Table offsets count int32 entries of the pool: xmin [T], count [T], then the weights TRANSPOSED,
// [ksize][T], so that neighbouring outputs read neighbouring words.  The horizontal xmin are input columns; the vertical ymin are
// relative to row0 (rows of the intermediate).
struct IngestImage {
    long long in_off;        // bytes into the pixel buffer
    long long inter_off;     // bytes into the intermediate
    int width, channels;
    int row0, nrows;         // input rows the window's vertical taps touch
    int h_off, h_ksize;
    int v_off, v_ksize;
};

struct IngestArgs {
    const uint8_t* pixels;
    long long pixels_bytes;
    const IngestImage* images;
    const int* pool;
    const uint8_t* white;    // [256 alpha][256 colour]
    uint8_t* inter;
    float* out;
    uint8_t* out_u8;         // nullable
    int T;
};

__global__ __launch_bounds__(INGEST_HC* INGEST_HR) void k_ingest_h(IngestArgs a) {
    __shared__ __attribute__((aligned(8))) uint8_t seg[INGEST_HR][INGEST_ROW_BYTES];
    const IngestImage d = a.images[blockIdx.z];
    const int x_first = blockIdx.x * INGEST_HC, r_first = blockIdx.y * INGEST_HR;
    if (x_first >= a.T || r_first >= d.nrows) return;
    const int t = threadIdx.x, ch = d.channels;
    const int* xmin = a.pool + d.h_off;
    const int* cnt = xmin + a.T;
    const int* kt = cnt + a.T;
    const int x_last = min(x_first + INGEST_HC, a.T) - 1;
    const int p_begin = xmin[x_first], p_end = xmin[x_last] + cnt[x_last];      // input columns this workgroup's outputs touch
    const int xo = x_first + (t & (INGEST_HC - 1)), rr = t >> 6;
    const bool live = xo <= x_last && r_first + rr < d.nrows;
    int my_min = 0, my_cnt = 0;
    if (live) { my_min = xmin[xo]; my_cnt = cnt[xo]; }
    int acc[3] = {1 << (INGEST_BITS - 1), 1 << (INGEST_BITS - 1), 1 << (INGEST_BITS - 1)};

    for (int tp0 = p_begin; tp0 < p_end; tp0 += INGEST_TILE) {
        const int tp1 = min(tp0 + INGEST_TILE, p_end);
        if (tp0 != p_begin) __syncthreads();
        // stage: dwords from the 4-byte boundary at or below the segment's first byte; a dword that would cross the end of the
        // pixel buffer is read byte by byte
        for (int r = 0; r < INGEST_HR; ++r) {
            if (r_first + r >= d.nrows) break;
            const long long b0 = d.in_off + ((long long)(d.row0 + r_first + r) * d.width + tp0) * ch;
            const long long b1 = b0 + (long long)(tp1 - tp0) * ch;
            const long long w0 = b0 >> 2, w1 = (b1 + 3) >> 2;
            for (long long w = w0 + t; w < w1; w += INGEST_HC * INGEST_HR) {
                unsigned v;
                if (w * 4 + 4 <= a.pixels_bytes) {
                    v = *reinterpret_cast<const unsigned*>(a.pixels + w * 4);
                } else {
                    v = 0;
                    for (int j = 0; j < 4; ++j)
                        if (w * 4 + j < a.pixels_bytes) v |= (unsigned)a.pixels[w * 4 + j] << (8 * j);
                }
                *reinterpret_cast<unsigned*>(&seg[r][(w - w0) * 4]) = v;
            }
        }
        __syncthreads();
        if (ch == 4) {      // blend over white in place: colour bytes only, the alpha byte stays
            for (int r = 0; r < INGEST_HR; ++r) {
                if (r_first + r >= d.nrows) break;
                const int mis = (int)((d.in_off + ((long long)(d.row0 + r_first + r) * d.width + tp0) * 4) & 3);
                for (int p = t; p < tp1 - tp0; p += INGEST_HC * INGEST_HR) {
                    uint8_t* px = &seg[r][mis + p * 4];
                    const uint8_t* row = a.white + (int)px[3] * 256;
                    px[0] = row[px[0]];
                    px[1] = row[px[1]];
                    px[2] = row[px[2]];
                }
            }
            __syncthreads();
        }
        if (live) {
            const int mis = (int)((d.in_off + ((long long)(d.row0 + r_first + rr) * d.width + tp0) * ch) & 3);
            const int j0 = max(my_min, tp0) - my_min, j1 = min(my_min + my_cnt, tp1) - my_min;
            for (int j = j0; j < j1; ++j) {
                const int k = kt[(long long)j * a.T + xo];
                const uint8_t* px = &seg[rr][mis + (my_min + j - tp0) * ch];
                acc[0] += (int)px[0] * k;
                acc[1] += (int)px[1] * k;
                acc[2] += (int)px[2] * k;
            }
        }
    }
    if (live) {
        uint8_t* o = a.inter + d.inter_off + ((long long)(r_first + rr) * a.T + xo) * 3;
        for (int c = 0; c < 3; ++c) o[c] = (uint8_t)min(max(acc[c] >> INGEST_BITS, 0), 255);
    }
}

__global__ __launch_bounds__(256) void k_ingest_v(IngestArgs a) {
    const IngestImage d = a.images[blockIdx.z];
    const int T = a.T;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (long long)T * T) return;
    const int y = (int)(pix / T), x = (int)(pix % T);
    const int* ymin = a.pool + d.v_off;
    const int* cnt = ymin + T;
    const int* kt = cnt + T;
    const int r0 = ymin[y], n = cnt[y];
    int acc[3] = {1 << (INGEST_BITS - 1), 1 << (INGEST_BITS - 1), 1 << (INGEST_BITS - 1)};
    const uint8_t* col = a.inter + d.inter_off + ((long long)r0 * T + x) * 3;
    for (int j = 0; j < n; ++j) {
        const int k = kt[(long long)j * T + y];
        const uint8_t* px = col + (long long)j * T * 3;
        acc[0] += (int)px[0] * k;
        acc[1] += (int)px[1] * k;
        acc[2] += (int)px[2] * k;
    }
    const long long img = blockIdx.z, TT = (long long)T * T;
    for (int c = 0; c < 3; ++c) {
        const int u = min(max(acc[c] >> INGEST_BITS, 0), 255);
        a.out[(img * 3 + c) * TT + (long long)y * T + x] = ingest_exit.v[u];
        if (a.out_u8) a.out_u8[(img * TT + (long long)y * T + x) * 3 + c] = (uint8_t)u;
    }
}

namespace {

double ingest_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return std::sin(x) / x;
}

double ingest_lanczos(double x) { return (-3.0 <= x && x < 3.0) ? ingest_sinc(x) * ingest_sinc(x / 3.0) : 0.0; }

// Pillow's bilinear_filter (Resample.c): the triangle 1 - |x| on |x| < 1
double ingest_bilinear(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

bool ingest_filter_ok(int filter) { return filter == WMAR_RESAMPLE_LANCZOS || filter == WMAR_RESAMPLE_BILINEAR; }
// the filter's support (Resample.c: LANCZOS 3.0, BILINEAR 1.0)
double ingest_support(int filter) { return filter == WMAR_RESAMPLE_BILINEAR ? 1.0 : 3.0; }

int ingest_ksize(int in_size, int out_size, int filter) {
    const double scale = (double)in_size / (double)out_size, filterscale = scale < 1.0 ? 1.0 : scale;
    return (int)std::ceil(ingest_support(filter) * filterscale) * 2 + 1;
}

// Tables of one axis for the outputs [out0, out0 + n_out); k row-major [n_out][ksize], zero beyond a row's count
void ingest_coeffs(int in_size, int out_size, int out0, int n_out, int32_t* xmin_out, int32_t* count_out, int32_t* k_out, int ksize,
                   int filter) {
    const double scale = (double)in_size / (double)out_size, filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = ingest_support(filter) * filterscale, ss = 1.0 / filterscale;      // the tap position is multiplied by the reciprocal
    std::vector<double> w((size_t)ksize);
    for (int i = 0; i < n_out; ++i) {
        const double center = ((double)(out0 + i) + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        const int count = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < count; ++x) {
            const double at = ((double)(x + xmin) - center + 0.5) * ss;
            w[x] = filter == WMAR_RESAMPLE_BILINEAR ? ingest_bilinear(at) : ingest_lanczos(at);
            ww += w[x];
        }
        int32_t* k = k_out + (size_t)i * ksize;
        for (int x = 0; x < ksize; ++x) {
            double v = x < count ? w[x] : 0.0;
            if (x < count && ww != 0.0) v /= ww;
            k[x] = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << INGEST_BITS)) : (int32_t)(0.5 + v * (double)(1 << INGEST_BITS));
        }
        xmin_out[i] = xmin;
        count_out[i] = count;
    }
}

const uint8_t* ingest_white_table() {
    static uint8_t table[65536];
    static std::once_flag once;
    std::call_once(once, [] {
        for (int al = 0; al < 256; ++al) {
            const double alpha = (double)al / 255.0;
            for (int c = 0; c < 256; ++c) table[al * 256 + c] = (uint8_t)((1 - alpha) * 255 + alpha * (double)c);
        }
    });
    return table;
}

// The call's device scratch, kept per device between calls and only ever grown: the whitening table (uploaded once per allocation),
// then the descriptors, the coefficient pool and the 8-bit intermediate of the current call.  A call holds the lock from its first
// use of the buffer until its launches have finished, so calls on one device take turns.
struct IngestScratch {
    uint8_t* buf = nullptr;
    size_t cap = 0;
};
std::mutex ingest_scratch_mutex;
std::map<int, IngestScratch> ingest_scratch;

// Appends one axis' device tables to the pool: xmin [T] (`rebase`: relative to the first one), count [T], weights [ksize][T].  An unchanged axis becomes
// the identity (one tap of weight 1.0, which the fixed-point arithmetic reproduces exactly): Pillow does not filter it.
void ingest_axis(std::vector<int32_t>& pool, int in_size, int out_size, int out0, int T, bool rebase, int filter, int* off, int* ksize_out,
                 int* first, int* end) {
    *off = (int)pool.size();
    if (in_size == out_size) {
        pool.resize(pool.size() + (size_t)3 * T);
        int32_t* p = pool.data() + *off;
        for (int i = 0; i < T; ++i) { p[i] = out0 + i; p[T + i] = 1; p[2 * T + i] = 1 << INGEST_BITS; }
        *ksize_out = 1;
        *first = out0;
        *end = out0 + T;
        if (rebase)
            for (int i = 0; i < T; ++i) p[i] -= out0;
        return;
    }
    const int ksize = ingest_ksize(in_size, out_size, filter);
    std::vector<int32_t> k((size_t)T * ksize);
    pool.resize(pool.size() + (size_t)T * (2 + ksize));
    int32_t* p = pool.data() + *off;
    ingest_coeffs(in_size, out_size, out0, T, p, p + T, k.data(), ksize, filter);
    for (int i = 0; i < T; ++i)
        for (int j = 0; j < ksize; ++j) p[2 * T + (size_t)j * T + i] = k[(size_t)i * ksize + j];
    *ksize_out = ksize;
    *first = p[0];
    *end = p[T - 1] + p[2 * T - 1];
    if (rebase)
        for (int i = T - 1; i >= 0; --i) p[i] -= p[0];
}

}  // namespace
}  // namespace wmar

using namespace wmar;

extern "C" int wmar_resample_coeffs_filtered(int32_t in_size, int32_t out_size, int32_t out0, int32_t n_out, int32_t* xmin_out,
                                             int32_t* count_out, int32_t* k_out, int32_t k_capacity, int32_t* ksize_out, int32_t filter) {
    WMAR_REQUIRE(ingest_filter_ok(filter), "resample_coeffs: filter %d (1 = LANCZOS, 2 = BILINEAR)", filter);
    WMAR_REQUIRE(in_size >= 1 && out_size >= 1, "resample_coeffs: sizes %d -> %d (both must be positive)", in_size, out_size);
    WMAR_REQUIRE(in_size <= INGEST_MAX_SIDE && out_size <= (1 << 30), "resample_coeffs: sizes %d -> %d beyond %d -> 2^30", in_size,
                 out_size, INGEST_MAX_SIDE);
    WMAR_REQUIRE(out0 >= 0 && n_out >= 1 && (long long)out0 + n_out <= out_size, "resample_coeffs: window [%d, %d + %d) outside %d outputs",
                 out0, out0, n_out, out_size);
    WMAR_REQUIRE(xmin_out && count_out && k_out && ksize_out, "resample_coeffs: null output");
    const int ksize = ingest_ksize(in_size, out_size, filter);
    WMAR_REQUIRE((long long)n_out * ksize <= k_capacity, "resample_coeffs: %lld coefficients, capacity %d", (long long)n_out * ksize,
                 k_capacity);
    ingest_coeffs(in_size, out_size, out0, n_out, xmin_out, count_out, k_out, ksize, filter);
    *ksize_out = ksize;
    return WMAR_OK;
}

extern "C" int wmar_resample_coeffs(int32_t in_size, int32_t out_size, int32_t out0, int32_t n_out, int32_t* xmin_out,
                                    int32_t* count_out, int32_t* k_out, int32_t k_capacity, int32_t* ksize_out) {
    return wmar_resample_coeffs_filtered(in_size, out_size, out0, n_out, xmin_out, count_out, k_out, k_capacity, ksize_out, WMAR_RESAMPLE_LANCZOS);
}

extern "C" int wmar_image_ingest_filtered(const uint8_t* pixels_dev, int64_t pixels_bytes, const wmar_image_desc* desc_host, int64_t n,
                                          int32_t target, float* out_dev, uint8_t* out_u8_dev, int32_t filter, void* stream) {
    WMAR_REQUIRE(ingest_filter_ok(filter), "image_ingest: filter %d (1 = LANCZOS, 2 = BILINEAR)", filter);
    WMAR_REQUIRE(pixels_dev && desc_host && out_dev && pixels_bytes >= 1, "image_ingest: bad argument");
    WMAR_REQUIRE(n >= 1 && n <= 65535, "image_ingest: %lld images (1..65535 per call)", (long long)n);
    WMAR_REQUIRE(target >= 1 && target <= INGEST_MAX_SIDE, "image_ingest: target %d (1..%d)", target, INGEST_MAX_SIDE);
    WMAR_REQUIRE(((uintptr_t)pixels_dev & 3) == 0, "image_ingest: the pixel buffer must be 4-byte aligned");
    const int T = target;
    std::vector<IngestImage> images((size_t)n);
    std::vector<int32_t> pool;
    std::map<std::tuple<int, int, int, int>, std::tuple<int, int, int, int>> axes;      // (axis, in, out, out0) -> (offset, ksize, first, end)
    long long inter_bytes = 0;
    int max_rows = 0;
    for (int64_t i = 0; i < n; ++i) {
        const wmar_image_desc& s = desc_host[i];
        WMAR_REQUIRE(s.channels == 3 || s.channels == 4, "image_ingest: image %lld has %d channels (3 = RGB, 4 = RGBA)", (long long)i,
                     s.channels);
        WMAR_REQUIRE(s.width >= 1 && s.height >= 1 && s.width <= INGEST_MAX_SIDE && s.height <= INGEST_MAX_SIDE,
                     "image_ingest: image %lld is %d x %d (sides 1..%d)", (long long)i, s.width, s.height, INGEST_MAX_SIDE);
        const long long bytes = (long long)s.width * s.height * s.channels;
        WMAR_REQUIRE(s.offset >= 0 && s.offset <= pixels_bytes && bytes <= pixels_bytes - s.offset,
                     "image_ingest: image %lld (%lld bytes at offset %lld) lies outside the %lld-byte pixel buffer", (long long)i, bytes,
                     (long long)s.offset, (long long)pixels_bytes);
        WMAR_REQUIRE(s.new_width >= 1 && s.new_height >= 1 && s.new_width <= (1 << 30) && s.new_height <= (1 << 30),
                     "image_ingest: image %lld resized to %d x %d", (long long)i, s.new_width, s.new_height);
        WMAR_REQUIRE(s.crop_x0 >= 0 && s.crop_y0 >= 0 && (long long)s.crop_x0 + T <= s.new_width && (long long)s.crop_y0 + T <= s.new_height,
                     "image_ingest: image %lld: crop window %d x %d at (%d, %d) outside the %d x %d resized image", (long long)i, T, T,
                     s.crop_x0, s.crop_y0, s.new_width, s.new_height);
        WMAR_REQUIRE((long long)T * (2 + ingest_ksize(s.width, s.new_width, filter)) + (long long)T * (2 + ingest_ksize(s.height, s.new_height, filter)) +
                             (long long)pool.size() < (1LL << 30),
                     "image_ingest: coefficient tables of the batch too large");
        IngestImage& d = images[(size_t)i];
        d.in_off = s.offset;
        d.width = s.width;
        d.channels = s.channels;
        int first = 0, end = 0;
        for (int axis = 0; axis < 2; ++axis) {
            const auto key = axis == 0 ? std::make_tuple(0, s.width, s.new_width, s.crop_x0) : std::make_tuple(1, s.height, s.new_height, s.crop_y0);
            auto it = axes.find(key);
            if (it == axes.end()) {
                int off, ks;
                ingest_axis(pool, std::get<1>(key), std::get<2>(key), std::get<3>(key), T, axis == 1, filter, &off, &ks, &first, &end);
                it = axes.emplace(key, std::make_tuple(off, ks, first, end)).first;
            }
            if (axis == 0) { d.h_off = std::get<0>(it->second); d.h_ksize = std::get<1>(it->second); }
            else { d.v_off = std::get<0>(it->second); d.v_ksize = std::get<1>(it->second); }
            first = std::get<2>(it->second);
            end = std::get<3>(it->second);
        }
        d.row0 = first;                  // of the vertical axis (handled last)
        d.nrows = end - first;
        d.inter_off = inter_bytes;
        inter_bytes += (long long)d.nrows * T * 3;
        if (d.nrows > max_rows) max_rows = d.nrows;
    }
    const long long gx = (T + INGEST_HC - 1) / INGEST_HC, gy = (max_rows + INGEST_HR - 1) / INGEST_HR;
    WMAR_REQUIRE(gx * gy * n * (INGEST_HC * INGEST_HR) < (1LL << 32) && ((long long)T * T + 255) / 256 * 256 * n < (1LL << 32),
                 "image_ingest: batch too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    const size_t img_bytes = images.size() * sizeof(IngestImage), pool_bytes = pool.size() * 4;
    const size_t o_white = 0, o_img = 65536, o_pool = o_img + (img_bytes + 255) / 256 * 256;
    const size_t o_inter = o_pool + (pool_bytes + 255) / 256 * 256, total = o_inter + (size_t)inter_bytes;
    int device = 0;
    WMAR_HIP_CHECK(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(ingest_scratch_mutex);
    IngestScratch& sc = ingest_scratch[device];
    if (sc.cap < total) {      // earlier calls have finished (each waits for its launches): the old buffer is idle
        if (sc.buf) (void)hipFree(sc.buf);
        sc.buf = nullptr;
        sc.cap = 0;
        const size_t want = (total + (size_t)(1 << 20) - 1) >> 20 << 20;
        if (hipMalloc((void**)&sc.buf, want) != hipSuccess) {
            sc.buf = nullptr;
            set_error("image_ingest: hipMalloc of %zu bytes of scratch failed", want);
            return WMAR_ENOMEM;
        }
        sc.cap = want;
        WMAR_HIP_CHECK(hipMemcpy(sc.buf + o_white, ingest_white_table(), 65536, hipMemcpyHostToDevice));
    }
    uint8_t* scratch = sc.buf;
    WMAR_HIP_CHECK(hipMemcpyAsync(scratch + o_img, images.data(), img_bytes, hipMemcpyHostToDevice, st));
    WMAR_HIP_CHECK(hipMemcpyAsync(scratch + o_pool, pool.data(), pool_bytes, hipMemcpyHostToDevice, st));
    IngestArgs a{};
    a.pixels = pixels_dev; a.pixels_bytes = pixels_bytes; a.images = (const IngestImage*)(scratch + o_img);
    a.pool = (const int*)(scratch + o_pool); a.white = scratch + o_white; a.inter = scratch + o_inter;
    a.out = out_dev; a.out_u8 = out_u8_dev; a.T = T;
    const dim3 gh((unsigned)gx, (unsigned)gy, (unsigned)n);
    hipLaunchKernelGGL(k_ingest_h, gh, dim3(INGEST_HC * INGEST_HR), 0, st, a);
    int rc = launch_status("k_ingest_h");
    if (rc == WMAR_OK) {
        const dim3 gv((unsigned)(((long long)T * T + 255) / 256), 1, (unsigned)n);
        hipLaunchKernelGGL(k_ingest_v, gv, dim3(256), 0, st, a);
        rc = launch_status("k_ingest_v");
    }
    // the tables were copied from this call's own host vectors and the scratch is handed to the next call: wait for the launches
    const hipError_t e = hipStreamSynchronize(st);
    if (rc == WMAR_OK && e != hipSuccess) {
        set_error("image_ingest: %s", hipGetErrorString(e));
        rc = WMAR_EHIP;
    }
    return rc;
}

extern "C" int wmar_image_ingest(const uint8_t* pixels_dev, int64_t pixels_bytes, const wmar_image_desc* desc_host, int64_t n,
                                 int32_t target, float* out_dev, uint8_t* out_u8_dev, void* stream) {
    return wmar_image_ingest_filtered(pixels_dev, pixels_bytes, desc_host, n, target, out_dev, out_u8_dev, WMAR_RESAMPLE_LANCZOS, stream);
}
