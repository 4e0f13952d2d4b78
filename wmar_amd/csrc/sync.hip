// The geometry fit of the synchronisation layer ("FT + Augs + Sync", wmar/watermarking/synchronization.py) as HIP kernels over the
// WHOLE batch: per-pixel message labels from the WAM predictions (estimate_augmentation_with_wam :224-243), and fit_best_aug +
// rotate_wm + find_cut (:90-201): the four label masks rotated by the 41 angles -20..20, thresholded, counted along both axes, and the
// cut / flip search per angle.  The reference does this on the host, 2.3 s per 256 x 256 image, once per (transform, parameter) pair.
//
// What is restated, and must decide every pixel as the reference does (tests/golden/sync_vectors.npz holds its outputs):
//   scipy.ndimage.rotate(mask, angle, reshape=False), mask = 0/255 int64, defaults order=3, mode="constant", cval=0, prefilter=True:
//     spline_filter      cubic B-spline prefilter in fp64 along axis 0 then axis 1: gain (1 - z)(1 - 1/z), pole z = sqrt(3) - 2,
//                        causal + anticausal recursion with the MIRROR initialisation (what scipy uses for mode="constant")
//     affine_transform   source coordinate of output (i, j): (i c + j s + o0, -i s + j c + o1), o = ctr - R ctr, ctr = (S - 1) / 2;
//                        a coordinate outside [0, S - 1] gives cval; else taps floor(x) - 1 .. floor(x) + 2 per axis (indices
//                        mirrored about 0 and S - 1), cubic B-spline weights, the 16 products summed in fp64
//     int64 output       the value is rounded to the nearest integer; with the reference's `>= 0.5` that is "fp64 value >= 0.5"
//   The prefilter does not depend on the angle: it runs once per (image, label); the 41 angles sample the same coefficients.
//   Compiled with -ffp-contract=off: scipy's C is not contracted either.  The fixtures keep every value 1e-10 away from 0.5; the
//   summation carries ~5e-13.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace wmar {

constexpr int SYNC_ANGLES = 41;          // -20 .. 20
constexpr int SYNC_MAX_S = 512;          // two columns per thread of the 256-thread angle kernel; 16 KiB of counters in LDS

// ---------------------------------------------------------------------------------------------------------------- positions
// one thread per pixel: 32 bits, Hamming distance to 0^32, 0^16 1^16, 1^16 0^16, 1^32 (first minimum wins, as torch.argmin), kept when
// the distance is <= 6 and fp32 sigmoid(mask logit) > 0.5 -- evaluated, not replaced by `logit > 0`: 1 / (1 + exp(-5e-8)) is 0.5
__global__ __launch_bounds__(256) void k_sync_positions(const float* __restrict__ preds, int8_t* __restrict__ positions,
                                                        int32_t* __restrict__ sizes, long long B, int S) {
    const long long HW = (long long)S * S;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    int lab = -1;
    long long b = 0;
    if (idx < B * HW) {
        b = idx / HW;
        const float* p = preds + b * 33 * HW + (idx - b * HW);
        unsigned bits = 0;
        for (int k = 0; k < 32; ++k) bits |= (p[(k + 1) * HW] > 0.f ? 1u : 0u) << k;      // bit k of the message = channel 1 + k
        const int lo = __popc(bits & 0xffffu), hi = __popc(bits >> 16);                   // ones among the first / last 16 bits
        const int d[4] = {lo + hi, lo + 16 - hi, 16 - lo + hi, 32 - lo - hi};
        int best = 0;
        for (int m = 1; m < 4; ++m) best = d[m] < d[best] ? m : best;
        const float sg = 1.0f / (1.0f + expf(-p[0]));
        lab = (d[best] <= 6 && sg > 0.5f) ? best : -1;
        positions[idx] = (int8_t)lab;
    }
    // sizes[b, m]: a wave's lanes may span two images only when HW is no multiple of 64; count per lane's own image
    for (int m = 0; m < 4; ++m) {
        if (HW % 64 == 0) {
            const unsigned long long v = __ballot(lab == m);
            if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sizes[b * 4 + m], (int)__popcll(v));
        } else if (lab == m) {
            atomicAdd(&sizes[b * 4 + m], 1);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- prefilter
struct SyncPre {
    const int8_t* pos;      // [nb, S, S]
    double* coef;           // [nb, S, S, 4]: the four labels' spline coefficients interleaved (one 32-byte read per tap)
    long long nb;
    int S;
    double z, gain, zn1;    // pole, (1 - z)(1 - 1/z), z^(S - 1)
};

// scipy's 1-D filter of one line: `load(i)` is the gain-scaled input, the line is written to out[i * stride]
template <class Load>
__device__ __forceinline__ void sync_filter_line(Load load, double* out, long long stride, int n, double z, double zn1) {
    double acc = load(0) + zn1 * load(n - 1);
    double zi = z;
    for (int i = 1; i < n - 1; ++i) {
        acc = acc + zi * (load(i) + zn1 * load(n - 1 - i));
        zi *= z;
    }
    double c = acc / (1.0 - zn1 * zn1);
    out[0] = c;
    for (int i = 1; i < n; ++i) {
        c = load(i) + z * c;
        out[i * stride] = c;
    }
    c = (z * out[(n - 2) * stride] + out[(n - 1) * stride]) * z / (z * z - 1.0);
    out[(n - 1) * stride] = c;
    for (int i = n - 2; i >= 0; --i) {
        c = z * (c - out[i * stride]);
        out[i * stride] = c;
    }
}

// axis 0: one thread per (image, column, label), reading the label map itself
__global__ __launch_bounds__(64) void k_sync_prefilter_cols(SyncPre a) {
    const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
    if (t >= a.nb * a.S * 4) return;
    const int l = (int)(t & 3), S = a.S;
    const int j = (int)((t >> 2) % S);
    const long long b = (t >> 2) / S;
    const int8_t* p = a.pos + b * S * S + j;
    const double on = 255.0 * a.gain;
    sync_filter_line([&](int i) { return p[(long long)i * S] == l ? on : 0.0; }, a.coef + (b * S * S + j) * 4 + l, (long long)S * 4, S,
                     a.z, a.zn1);
}
// axis 1: one thread per (image, row, label), in place
__global__ __launch_bounds__(64) void k_sync_prefilter_rows(SyncPre a) {
    const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
    if (t >= a.nb * a.S * 4) return;
    const int l = (int)(t & 3), S = a.S;
    double* line = a.coef + (t >> 2) * S * 4 + l;          // (t >> 2) = b * S + i
    const double g = a.gain;
    sync_filter_line([&](int i) { return line[i * 4] * g; }, line, 4, S, a.z, a.zn1);
}

// ---------------------------------------------------------------------------------------------------------------- rotation
struct SyncRot {
    double cs[SYNC_ANGLES], sn[SYNC_ANGLES], o0[SYNC_ANGLES], o1[SYNC_ANGLES];
};

__device__ __forceinline__ void sync_weights(double t, double w[4]) {
    const double z = 1.0 - t;
    w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
    w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
    w[0] = z * z * z / 6.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
}
__device__ __forceinline__ int sync_mirror(int i, int n) {
    i = i < 0 ? -i : i;
    return i > n - 1 ? 2 * (n - 1) - i : i;
}
// merged label (0 = background, 1..4; the later label overwrites) of output pixel (i, j) of image `coef` [S, S, 4]
__device__ __forceinline__ int sync_label(const double* __restrict__ coef, int S, int i, int j, double c, double s, double o0, double o1) {
    const double y = (double)i * c + (double)j * s + o0;
    const double x = (double)i * (-s) + (double)j * c + o1;
    const double hi = (double)(S - 1);
    if (y < 0.0 || y > hi || x < 0.0 || x > hi) return 0;
    const double fy = floor(y), fx = floor(x);
    double wy[4], wx[4];
    sync_weights(y - fy, wy);
    sync_weights(x - fx, wx);
    int iy[4], ix[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        iy[k] = sync_mirror((int)fy - 1 + k, S);
        ix[k] = sync_mirror((int)fx - 1 + k, S);
    }
    double t[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const double2* q = reinterpret_cast<const double2*>(coef + ((long long)iy[a] * S + ix[b]) * 4);
            const double2 v01 = q[0], v23 = q[1];
            t[0] += v01.x * wy[a] * wx[b];
            t[1] += v01.y * wy[a] * wx[b];
            t[2] += v23.x * wy[a] * wx[b];
            t[3] += v23.y * wy[a] * wx[b];
        }
    }
    return t[3] >= 0.5 ? 4 : t[2] >= 0.5 ? 3 : t[1] >= 0.5 ? 2 : t[0] >= 0.5 ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_sync_rotate_map(const double* __restrict__ coef, uint8_t* __restrict__ out, long long nb, int S,
                                                         double c, double s, double o0, double o1) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nb * S * S) return;
    const int j = (int)(idx % S), i = (int)((idx / S) % S);
    const long long b = idx / ((long long)S * S);
    out[idx] = (uint8_t)sync_label(coef + b * S * S * 4, S, i, j, c, s, o0, o1);
}

// ---------------------------------------------------------------------------------------------------------------- one angle
struct SyncFit {
    const double* coef;     // this chunk's coefficients
    double* err;            // [B, 41] of the whole batch
    int32_t* cut;           // [B, 41, 3]: cut_i, cut_j, flipped
    long long b0;           // first image of the chunk
    int S, thresh;
    SyncRot r;
};

struct SyncScan { int mn, count, first, last; };

// find_cut (:99-162) of one dimension from the eight scans' results; c[l] = the cumulative counts of label l + 1 along this dimension
__device__ void sync_find_cut(const int* const c[4], const SyncScan* scan, int pl0, int pr0, int pl1, int pr1, bool dim1, int S,
                              double* err, int* cut_out, int* flip_out) {
    const int pl[2] = {pl0, pl1}, pr[2] = {pr0, pr1};
    long long cut = 0, cut_weight = 0;
    int votes = 0;
    for (int p = 0; p < 2; ++p) {
        const SyncScan n = scan[2 * p], f = scan[2 * p + 1];
        const int tl = c[pl[p]][S - 1], tr = c[pr[p]][S - 1];
        const double score_n = (double)n.mn - (double)n.count * 1e-3, score_f = (double)f.mn - (double)f.count * 1e-3;
        const bool fl = !(score_n < score_f || dim1);
        votes += fl ? 1 : -1;
        const SyncScan m = fl ? f : n;
        int pick;
        if (tr != 0 && tl == 0) pick = fl ? m.first : m.last;          // only R exists
        else if (tl != 0 && tr == 0) pick = fl ? m.last : m.first;     // only L exists
        else pick = (m.first + m.last) / 2;
        const long long w = (long long)tl + tr;
        cut += (long long)pick * w;
        cut_weight += w;
    }
    if (cut_weight == 0) { *err = 1e9; *cut_out = S / 2; *flip_out = 0; return; }
    const int at = (int)rint((double)cut / (double)cut_weight);       // Python's round(): half to even
    const bool flipped = ((double)votes / (double)cut_weight) > 0.0;
    long long e = 0;
    for (int p = 0; p < 2; ++p) {
        const int* cl = c[pl[p]];
        const int* cr = c[pr[p]];
        e += flipped ? cl[at] + (cr[S - 1] - cr[at]) : cr[at] + (cl[S - 1] - cl[at]);
    }
    *err = (double)e; *cut_out = at; *flip_out = flipped ? 1 : 0;
}

// One workgroup per (angle, image).  Thread t owns columns t and t + 256: their per-label counts stay in registers over the rows;
// a row's per-label counts are wave ballots added to LDS (integer atomics: no order dependence).  Then the threshold, the cumulative
// sums (8 threads), the 8 error-curve scans (8 threads) and the cut logic (1 thread).
__global__ __launch_bounds__(256) void k_sync_angle(SyncFit a) {
    __shared__ int cnt[2][4][SYNC_MAX_S];        // [0]: per column (np.sum(axis=0)), [1]: per row
    __shared__ SyncScan scan[8];
    const int S = a.S, ang = blockIdx.x, tid = threadIdx.x;
    const long long bl = blockIdx.y;             // image within the chunk
    const double* coef = a.coef + bl * S * S * 4;
    for (int k = tid; k < 4 * SYNC_MAX_S; k += 256) (&cnt[1][0][0])[k] = 0;
    __syncthreads();
    const double c = a.r.cs[ang], s = a.r.sn[ang], o0 = a.r.o0[ang], o1 = a.r.o1[ang];
    int cc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    const int ncol = (S + 255) / 256;            // 1 or 2, the same for every thread
    for (int i = 0; i < S; ++i) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k < ncol) {
                const int j = tid + 256 * k;
                const int lab = j < S ? sync_label(coef, S, i, j, c, s, o0, o1) : 0;
#pragma unroll
                for (int l = 1; l <= 4; ++l) {
                    cc[k][l - 1] += lab == l ? 1 : 0;
                    const unsigned long long v = __ballot(lab == l);
                    if ((tid & 63) == 0 && v) atomicAdd(&cnt[1][l - 1][i], (int)__popcll(v));
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int j = tid + 256 * k;
        if (j < S)
            for (int l = 0; l < 4; ++l) cnt[0][l][j] = cc[k][l];
    }
    __syncthreads();
    if (tid < 8) {          // counts below the threshold are dropped, then np.cumsum
        int* q = cnt[tid >> 2][tid & 3];
        int run = 0;
        for (int k = 0; k < S; ++k) {
            const int v = q[k];
            run += v < a.thresh ? 0 : v;
            q[k] = run;
        }
    }
    __syncthreads();
    if (tid < 8) {          // scans 0..3: dim 1 (rows), pairs (1, 3) and (2, 4); 4..7: dim 0 (columns), pairs (1, 2) and (3, 4); odd = flipped curve
        const int dim = tid < 4 ? 1 : 0, p = (tid >> 1) & 1;
        const int l = dim ? p : 2 * p, r = dim ? p + 2 : 2 * p + 1;      // label - 1
        const int* cl = cnt[dim][l];
        const int* cr = cnt[dim][r];
        const bool fl = tid & 1;
        const int tl = cl[S - 1], tr = cr[S - 1];
        SyncScan m = {0x7fffffff, 0, 0, 0};
        for (int k = 0; k < S; ++k) {
            const int e = fl ? cl[k] + (tr - cr[k]) : cr[k] + (tl - cl[k]);
            if (e < m.mn) { m.mn = e; m.count = 1; m.first = k; m.last = k; }
            else if (e == m.mn) { ++m.count; m.last = k; }
        }
        scan[tid] = m;
    }
    __syncthreads();
    if (tid == 0) {
        const int* rows[4] = {cnt[1][0], cnt[1][1], cnt[1][2], cnt[1][3]};
        const int* cols[4] = {cnt[0][0], cnt[0][1], cnt[0][2], cnt[0][3]};
        double ei, ej;
        int cuti, cutj, fi, fj;
        sync_find_cut(rows, scan, 0, 2, 1, 3, true, S, &ei, &cuti, &fi);
        sync_find_cut(cols, scan + 4, 0, 1, 2, 3, false, S, &ej, &cutj, &fj);
        const long long o = (a.b0 + bl) * SYNC_ANGLES + ang;
        a.err[o] = ei + ej;
        a.cut[o * 3 + 0] = cuti; a.cut[o * 3 + 1] = cutj; a.cut[o * 3 + 2] = fj;
    }
}

// selection across the angles (:171-201): a strictly smaller error replaces the cuts and the list of best angles, an equal one
// extends the list; the rotation is round((max + min) / 2), half to even.  One thread per image.
__global__ __launch_bounds__(64) void k_sync_select(const double* __restrict__ err, const int32_t* __restrict__ cut, int32_t* __restrict__ aug,
                                                    double* __restrict__ total_error, long long B, int S) {
    const long long b = (long long)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double best = INFINITY;
    int lo = 0, hi = 0, ci = S / 2, cj = S / 2, fl = 0;
    for (int n = 0; n < SYNC_ANGLES; ++n) {
        const double e = err[b * SYNC_ANGLES + n];
        const int angle = n - 20;
        if (total_error) total_error[b * SYNC_ANGLES + n] = e;
        if (e < best) {
            best = e; lo = hi = angle;
            ci = cut[(b * SYNC_ANGLES + n) * 3]; cj = cut[(b * SYNC_ANGLES + n) * 3 + 1]; fl = cut[(b * SYNC_ANGLES + n) * 3 + 2];
        } else if (e == best) {
            lo = angle < lo ? angle : lo; hi = angle > hi ? angle : hi;
        }
    }
    aug[b * 4 + 0] = (int)rint((double)(hi + lo) / 2.0);
    aug[b * 4 + 1] = ci; aug[b * 4 + 2] = cj; aug[b * 4 + 3] = fl;
}

// ---------------------------------------------------------------------------------------------------------------- host
static void sync_rotation(int angle, int S, double* c, double* s, double* o0, double* o1) {
    const double rad = (double)angle * 3.14159265358979323846 / 180.0;
    *c = cos(rad); *s = sin(rad);
    const double ctr = (double)(S - 1) / 2.0;
    *o0 = ctr - (*c * ctr + *s * ctr);
    *o1 = ctr - (-*s * ctr + *c * ctr);
}

static int64_t sync_result_bytes(int64_t B) { return ((B * SYNC_ANGLES * (8 + 12)) + 255) / 256 * 256; }
static int64_t sync_image_bytes(int32_t S) { return (int64_t)S * S * 4 * 8; }

static int sync_check(const void* positions_dev, int64_t B, int32_t S, const void* ws, int64_t ws_bytes, const char* who) {
    WMAR_REQUIRE(positions_dev && B >= 1, "%s: bad argument", who);
    WMAR_REQUIRE(S >= 4 && S <= SYNC_MAX_S, "%s: label maps of %d x %d pixels (square, 4..%d)", who, S, S, SYNC_MAX_S);
    WMAR_REQUIRE(B <= 65535, "%s: batch of %lld images (at most 65535 per call)", who, (long long)B);
    WMAR_REQUIRE(ws && ((uintptr_t)ws & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
    const int64_t least = sync_result_bytes(B) + sync_image_bytes(S);
    WMAR_REQUIRE(ws_bytes >= least, "%s: workspace of %lld bytes, at least %lld needed (%lld for one launch sequence)", who,
                 (long long)ws_bytes, (long long)least, (long long)(sync_result_bytes(B) + B * sync_image_bytes(S)));
    return WMAR_OK;
}

static int sync_prefilter(const int8_t* pos, double* coef, int64_t nb, int32_t S, hipStream_t st) {
    SyncPre p{};
    p.pos = pos; p.coef = coef; p.nb = nb; p.S = S;
    p.z = sqrt(3.0) - 2.0;
    p.gain = (1.0 - p.z) * (1.0 - 1.0 / p.z);
    p.zn1 = pow(p.z, (double)(S - 1));
    const unsigned grid = (unsigned)((nb * S * 4 + 63) / 64);
    hipLaunchKernelGGL(k_sync_prefilter_cols, dim3(grid), dim3(64), 0, st, p);
    if (int rc = launch_status("k_sync_prefilter_cols")) return rc;
    hipLaunchKernelGGL(k_sync_prefilter_rows, dim3(grid), dim3(64), 0, st, p);
    return launch_status("k_sync_prefilter_rows");
}

}  // namespace wmar

using namespace wmar;

extern "C" int wmar_sync_positions(const float* preds_dev, int64_t B, int32_t S, int8_t* positions_dev, int32_t* sizes_dev, void* stream) {
    WMAR_REQUIRE(preds_dev && positions_dev && sizes_dev && B >= 1 && S >= 1, "sync_positions: bad argument");
    const long long n = (long long)B * S * S;
    WMAR_REQUIRE((n + 255) / 256 < (1LL << 31), "sync_positions: batch too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    WMAR_HIP_CHECK(hipMemsetAsync(sizes_dev, 0, (size_t)B * 4 * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_sync_positions, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, preds_dev, positions_dev, sizes_dev,
                       (long long)B, (int)S);
    return launch_status("k_sync_positions");
}

extern "C" int64_t wmar_sync_workspace_bytes(int64_t B, int32_t S) {
    if (B < 1 || S < 1) return 0;
    return sync_result_bytes(B) + B * sync_image_bytes(S);
}

extern "C" int wmar_sync_fit(const int8_t* positions_dev, int64_t B, int32_t S, int32_t* aug_dev, double* total_error_dev,
                             void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (int rc = sync_check(positions_dev, B, S, workspace_dev, workspace_bytes, "sync_fit")) return rc;
    WMAR_REQUIRE(aug_dev, "sync_fit: bad argument");
    hipStream_t st = (hipStream_t)stream;
    SyncFit f{};
    f.err = (double*)workspace_dev;
    f.cut = (int32_t*)(f.err + B * SYNC_ANGLES);
    double* coef = (double*)((char*)workspace_dev + sync_result_bytes(B));
    f.coef = coef; f.S = S; f.thresh = S == 256 ? 40 : 80;
    for (int n = 0; n < SYNC_ANGLES; ++n) sync_rotation(n - 20, S, &f.r.cs[n], &f.r.sn[n], &f.r.o0[n], &f.r.o1[n]);
    const int64_t chunk = std::min<int64_t>(B, (workspace_bytes - sync_result_bytes(B)) / sync_image_bytes(S));
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {         // one pass when the workspace holds the batch's coefficients
        const int64_t nb = std::min(chunk, B - b0);
        if (int rc = sync_prefilter(positions_dev + b0 * S * S, coef, nb, S, st)) return rc;
        f.b0 = b0;
        hipLaunchKernelGGL(k_sync_angle, dim3(SYNC_ANGLES, (unsigned)nb), dim3(256), 0, st, f);
        if (int rc = launch_status("k_sync_angle")) return rc;
    }
    hipLaunchKernelGGL(k_sync_select, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, f.err, f.cut, aug_dev, total_error_dev,
                       (long long)B, (int)S);
    return launch_status("k_sync_select");
}

extern "C" int wmar_sync_rotate_labels(const int8_t* positions_dev, int64_t B, int32_t S, int32_t angle, uint8_t* out_dev,
                                       void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (int rc = sync_check(positions_dev, B, S, workspace_dev, workspace_bytes, "sync_rotate_labels")) return rc;
    WMAR_REQUIRE(out_dev && angle >= -180 && angle <= 180, "sync_rotate_labels: bad argument");
    hipStream_t st = (hipStream_t)stream;
    double* coef = (double*)((char*)workspace_dev + sync_result_bytes(B));
    double c, s, o0, o1;
    sync_rotation(angle, S, &c, &s, &o0, &o1);
    const int64_t chunk = std::min<int64_t>(B, (workspace_bytes - sync_result_bytes(B)) / sync_image_bytes(S));
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = std::min(chunk, B - b0);
        if (int rc = sync_prefilter(positions_dev + b0 * S * S, coef, nb, S, st)) return rc;
        const long long n = (long long)nb * S * S;
        hipLaunchKernelGGL(k_sync_rotate_map, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, coef, out_dev + b0 * S * S,
                           (long long)nb, (int)S, c, s, o0, o1);
        if (int rc = launch_status("k_sync_rotate_map")) return rc;
    }
    return WMAR_OK;
}
