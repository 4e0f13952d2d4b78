// Trainable VQGAN tokenizers (gfx950; Taming first, MaskGIT below): a forward that records a tape, and the backward of encoder + quant_conv and of post_quant_conv +
// decoder, built from the layer functions of vq_grad.h.  Included at the end of vqgan.hip behind vq_grad.h.
//
// Reference: deps/taming/models/vqgan.py:64-73 (encode / decode) under torch.autograd, as finetune.py trains them
// (deps/taming/models/vqgan.py:86-169).  Dropout is 0 and GroupNorm has no train mode: the training forward IS the inference forward.
//
// Each half is a list of operations written once at create time in the order wmar_vq_encode / wmar_vq_decode make their run_gn,
// run_conv and attn_core calls, so a training forward launches the same kernels on the same values and is bit-equal to the
// inference engine.  What differs is where results go: every layer output has a slot of its own (the tape) instead of four rotating
// buffers, every norm's (mean, rstd) is copied out of the shared table, every attention keeps its softmax.  The backward walks the list
// in reverse.  A gradient buffer that already holds a contribution (the input of a ResnetBlock: shortcut + norm1 path; the input of an
// AttnBlock: residual + q, k, v) gets the next one through a scratch buffer and an elementwise add -- stream order, no atomics.
// The convs behind one norm (q, k, v) add their input gradients into one buffer first; the norm's backward then runs once.
// All memory is allocated at create time for max_batch images.
//
// wmar_mvq_train_create builds the same handle for RAR's MaskGIT-VQGAN (deps/rar/modeling/modules/maskgit_vqgan.py, titok.py:91-208):
// a second pair of op lists in wmar_mvq_encode's / wmar_mvq_decode's order -- bias-free block convs, the 1 x 1 shortcut on the block
// output, average pools, no attention, no quant convs -- with the [-1, 1] <-> [0, 1] range change and the clamp differentiated at the
// image edges.
#pragma once

namespace wmar {

__global__ void k_add_into(float* __restrict__ dst, const float* __restrict__ src, long long n4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 a = ((float4*)dst)[i];
    const float4 b = ((const float4*)src)[i];
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    ((float4*)dst)[i] = a;
}

__global__ void k_add_into1(float* __restrict__ dst, const float* __restrict__ src, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

// y = GroupNorm(x) (+ swish) as the convs' patch loaders stage it (conv_gn_apply), materialised for the weight gradient
__global__ void k_gn_apply(const float* __restrict__ x, float* __restrict__ y, const float2* __restrict__ mr, const float* __restrict__ gamma,
                           const float* __restrict__ beta, long long total4, int HW, int C, int swish) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total4) return;
    const int q4 = C >> 2, cpg = C / 32;
    const int c = (int)(idx % q4) * 4;
    const long long pix = idx / q4;
    const int b = (int)(pix / HW);
    const float4 v = *(const float4*)(x + pix * C + c);
    const float vs[4] = {v.x, v.y, v.z, v.w};
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float2 m = mr[b * 32 + (c + i) / cpg];
        r[i] = (vs[i] - m.x) * m.y * gamma[c + i] + beta[c + i];
        if (swish) r[i] = r[i] / (1.0f + __expf(-r[i]));
    }
    *(float4*)(y + pix * C + c) = make_float4(r[0], r[1], r[2], r[3]);
}

// NHWC (stored Cs channels) -> NCHW first C channels, no clamp (VQModel.decode; the input gradient of the encoder)
__global__ void k_nhwc_to_nchw(const float* __restrict__ src, float* __restrict__ dst, int C, int HW, int Cs) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long b = blockIdx.y;
    if (idx >= HW) return;
    for (int c = 0; c < C; ++c) dst[((long long)b * C + c) * HW + idx] = src[((long long)b * HW + idx) * Cs + c];
}

}  // namespace wmar

namespace {

struct TTensor { float* d = nullptr; float* g = nullptr; int C = 0, H = 0; bool gset = false; size_t elems(int B) const { return (size_t)B * H * H * C; } };
struct TNorm { NormW n; float *dg = nullptr, *db = nullptr; float2* mr = nullptr; std::string name; };
struct TConv {
    ConvW fw, dg;                      // the forward's packed weights; the flipped, transposed ones of a stride-1 conv
    float *w = nullptr, *wt = nullptr;  // raw weight (the stride-2 gather reads it), flipped weight
    float *gw = nullptr, *gb = nullptr;
    int cin = 0, cout = 0, ks = 1, stride = 1;
    bool bias = true;                  // false: a bias-free conv (MaskGIT-VQGAN blocks, encoder.conv_in) -- no gb, no ".bias" gradient
    std::string name;
};
enum { T_GN = 0, T_CONV = 1, T_ATTN = 2, T_POOL = 3 };
struct TOp { int kind = 0, in = -1, out = -1, res = -1, conv = -1, norm = -1, swish = 0, up = 0, q = -1, k = -1, v = -1; float* P = nullptr; };
struct THalf { std::vector<TOp> ops; int first = -1, last = -1, B = 0; bool tape = false, grads = false; };
struct TGrad { float* p; size_t n; int half; };

}  // namespace

struct wmar_vq_train {
    wmar_vq_config cfg{};
    DeviceArena mem;
    int Bmax = 0, S = 0;
    bool mvq = false;                   // MaskGIT-VQGAN plan: images cross in [-1, 1], the range change and the clamp are differentiated
    std::vector<TTensor> t;
    std::vector<TNorm> norms;
    std::vector<TConv> convs;
    THalf half[2];                      // 0 = encoder + quant_conv, 1 = post_quant_conv + decoder
    std::map<std::string, TGrad> grad_of;
    // scratch
    double *gn_partial = nullptr, *gn_tiles = nullptr, *gnb = nullptr; long long gn_tiles_cap = 0;
    float *ybuf = nullptr, *ngy = nullptr, *gtmp = nullptr, *ups = nullptr, *ws = nullptr, *dp = nullptr, *tr = nullptr;
    u32x4 *attk = nullptr, *attv = nullptr; float* zbias = nullptr;
    size_t max_elems = 0, ups_elems = 0, ws_elems = 0, gnb_doubles = 0, attn_nn = 0, attn_nc = 0;
    bool ngy_set = false;
};

namespace {

// (re)pack a conv's forward and dgrad weights from a torch-layout weight and bias: Loader::conv without the allocations
int repack_conv(TConv& c, const float* W, const float* bias, hipStream_t st) {
    auto pack = [&](ConvW& p, const float* src, int cin, int cout, const float* b) {
        const int T = c.ks * c.ks;
        const size_t n = (size_t)p.CT * T * p.KBc * 64;
        hipLaunchKernelGGL(k_pack_conv, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, p.wp, cout, cin, c.ks, p.CT, p.KBc);
        if (b) hipLaunchKernelGGL(k_pad_vec, dim3((p.CT * 32 + 255) / 256), dim3(256), 0, st, b, p.bias, cout, p.CT * 32);
        if (p.wq) {
            const size_t nq = (size_t)p.CT * T * (p.cin_s / 16) * 64;
            hipLaunchKernelGGL(k_pack_conv_bx, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, src, p.wq, cout, cin, c.ks, p.CT, p.cin_s / 16);
        }
        if (p.wf) {
            const size_t nf = (size_t)p.cin_s * 9 * 4;
            hipLaunchKernelGGL(k_pack_conv_few, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, src, p.wf, cout, cin, p.cin_s);
        }
    };
    const size_t nw = (size_t)c.cout * c.cin * c.ks * c.ks;
    WMAR_HIP_CHECK(hipMemcpyAsync(c.w, W, nw * 4, hipMemcpyDeviceToDevice, st));
    pack(c.fw, c.w, c.cin, c.cout, bias);
    if (c.stride == 1) {
        hipLaunchKernelGGL(k_flip_transpose_w, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, (const float*)c.w, c.wt, c.cout, c.cin, c.ks);
        pack(c.dg, c.wt, c.cout, c.cin, nullptr);      // zero bias stays zero
    }
    return launch_status("repack_conv");
}

struct TrainBuilder {
    wmar_vq_train* e;
    Loader& ld;
    hipStream_t st;
    int& rc;
    int tensor(int C, int H) {
        TTensor tt; tt.C = pad8(C); tt.H = H;
        WMAR_TRY(e->mem.alloc(&tt.d, tt.elems(e->Bmax)));
        WMAR_TRY(e->mem.alloc(&tt.g, tt.elems(e->Bmax)));
        if (tt.elems(e->Bmax) > e->max_elems) e->max_elems = tt.elems(e->Bmax);
        e->t.push_back(tt);
        return (int)e->t.size() - 1;
    }
    int norm(const std::string& name, int C, int hidx) {
        TNorm n; n.name = name;
        ld.norm(name, C, n.n);
        WMAR_TRY(e->mem.alloc(&n.dg, (size_t)C));
        WMAR_TRY(e->mem.alloc(&n.db, (size_t)C));
        WMAR_TRY(e->mem.alloc(&n.mr, (size_t)e->Bmax * 32));
        e->grad_of[name + ".weight"] = TGrad{n.dg, (size_t)C, hidx};
        e->grad_of[name + ".bias"] = TGrad{n.db, (size_t)C, hidx};
        e->norms.push_back(n);
        return (int)e->norms.size() - 1;
    }
    int conv(const std::string& name, int cin, int cout, int ks, int stride, int hidx, bool bias = true) {
        TConv c; c.name = name; c.cin = cin; c.cout = cout; c.ks = ks; c.stride = stride; c.bias = bias;
        const size_t nw = (size_t)cout * cin * ks * ks;
        ld.conv(name, cin, cout, ks, c.fw, bias);
        const float* W = ld.need(name + ".weight");
        WMAR_TRY(e->mem.alloc(&c.w, nw));
        WMAR_TRY(e->mem.alloc(&c.gw, nw));
        if (bias) WMAR_TRY(e->mem.alloc(&c.gb, (size_t)cout));
        if (rc == WMAR_OK && hipMemcpyAsync(c.w, W, nw * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { set_error("weight copy failed"); rc = WMAR_EHIP; }
        if (stride == 1 && rc == WMAR_OK) {
            WMAR_TRY(e->mem.alloc(&c.wt, nw));
            if (rc == WMAR_OK) {
                hipLaunchKernelGGL(k_flip_transpose_w, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, (const float*)c.w, c.wt, cout, cin, ks);
                const char* names[1] = {"dgrad.weight"};
                const void* tensors[1] = {c.wt};
                Loader l2(names, tensors, 1, &e->mem, st);
                l2.conv("dgrad", cout, cin, ks, c.dg, false);
                rc = l2.rc;
            }
        }
        e->grad_of[name + ".weight"] = TGrad{c.gw, nw, hidx};
        if (bias) e->grad_of[name + ".bias"] = TGrad{c.gb, (size_t)cout, hidx};
        e->convs.push_back(c);
        return (int)e->convs.size() - 1;
    }
    void op_gn(THalf& h, int in, int n, int swish) { TOp o; o.kind = T_GN; o.in = in; o.norm = n; o.swish = swish; h.ops.push_back(o); }
    // returns the output tensor
    int op_conv(THalf& h, int hidx, const std::string& name, int cin, int cout, int ks, int in, int res, int n, int swish, int stride, int up,
                bool bias = true) {
        const int Hin = e->t[in].H;
        const int Ho = up ? 2 * Hin : (stride == 2 ? Hin / 2 : Hin);
        TOp o; o.kind = T_CONV; o.in = in; o.res = res; o.norm = n; o.swish = swish; o.up = up;
        o.conv = conv(name, cin, cout, ks, stride, hidx, bias);
        o.out = tensor(cout, Ho);
        h.ops.push_back(o);
        if (up) { const size_t u = (size_t)e->Bmax * Ho * Ho * pad8(cin); if (u > e->ups_elems) e->ups_elems = u; }
        const size_t w = wgrad_ws_elems(e->Bmax * Ho * Ho, cout, cin, ks);
        if (w > e->ws_elems) e->ws_elems = w;
        return o.out;
    }
    int res(THalf& h, int hidx, const std::string& p, int cin, int cout, int X) {          // run_res
        const int H = e->t[X].H;
        const int n1 = norm(p + "norm1", cin, hidx);
        note_norm(cin, H);
        op_gn(h, X, n1, 1);
        const int T = op_conv(h, hidx, p + "conv1", cin, cout, 3, X, -1, n1, 1, 1, 0);
        const int n2 = norm(p + "norm2", cout, hidx);
        note_norm(cout, H);
        op_gn(h, T, n2, 1);
        int shortcut = X;
        if (cin != cout) shortcut = op_conv(h, hidx, p + "nin_shortcut", cin, cout, 1, X, -1, -1, 0, 1, 0);
        return op_conv(h, hidx, p + "conv2", cout, cout, 3, T, shortcut, n2, 1, 1, 0);
    }
    // run_mres: bias-free convs; out = h + nin_shortcut(h) with h = conv2(...) when cin != cout (a 1 x 1 conv whose input and residual
    // are the same tensor), else h + x
    int mres(THalf& h, int hidx, const std::string& p, int cin, int cout, int X) {
        const int H = e->t[X].H;
        const int n1 = norm(p + "norm1", cin, hidx);
        note_norm(cin, H);
        op_gn(h, X, n1, 1);
        const int T = op_conv(h, hidx, p + "conv1", cin, cout, 3, X, -1, n1, 1, 1, 0, false);
        const int n2 = norm(p + "norm2", cout, hidx);
        note_norm(cout, H);
        op_gn(h, T, n2, 1);
        if (cin != cout) {
            const int A = op_conv(h, hidx, p + "conv2", cout, cout, 3, T, -1, n2, 1, 1, 0, false);
            return op_conv(h, hidx, p + "nin_shortcut", cout, cout, 1, A, A, -1, 0, 1, 0, false);
        }
        return op_conv(h, hidx, p + "conv2", cout, cout, 3, T, X, n2, 1, 1, 0, false);
    }
    int op_pool(THalf& h, int in) {                                                          // k_avgpool2
        TOp o; o.kind = T_POOL; o.in = in;
        o.out = tensor(e->t[in].C, e->t[in].H / 2);
        h.ops.push_back(o);
        return o.out;
    }
    int attn(THalf& h, int hidx, const std::string& p, int c, int X) {                      // run_attn
        const int H = e->t[X].H;
        const int n = norm(p + "norm", c, hidx);
        note_norm(c, H);
        op_gn(h, X, n, 0);
        const int q = op_conv(h, hidx, p + "q", c, c, 1, X, -1, n, 0, 1, 0);
        const int k = op_conv(h, hidx, p + "k", c, c, 1, X, -1, n, 0, 1, 0);
        const int v = op_conv(h, hidx, p + "v", c, c, 1, X, -1, n, 0, 1, 0);
        TOp o; o.kind = T_ATTN; o.q = q; o.k = k; o.v = v; o.in = X;
        o.out = tensor(c, H);
        const size_t N = (size_t)H * H;
        WMAR_TRY(e->mem.alloc(&o.P, (size_t)e->Bmax * N * N));
        if ((size_t)e->Bmax * N * N > e->attn_nn) e->attn_nn = (size_t)e->Bmax * N * N;
        if ((size_t)e->Bmax * N * c > e->attn_nc) e->attn_nc = (size_t)e->Bmax * N * c;
        h.ops.push_back(o);
        return op_conv(h, hidx, p + "proj_out", c, c, 1, o.out, X, -1, 0, 1, 0);
    }
    void note_norm(int C, int H) {
        const size_t d = gnb_scratch_doubles(e->Bmax, H * H, C);
        if (d > e->gnb_doubles) e->gnb_doubles = d;
    }
};

// the buffers every plan shares, sized by what the builder noted; zbias_elems: the zeros attention reads as a bias
void train_scratch(wmar_vq_train* e, int& rc, size_t zbias_elems, hipStream_t st) {
    WMAR_TRY(e->mem.alloc(&e->ybuf, e->max_elems));
    WMAR_TRY(e->mem.alloc(&e->ngy, e->max_elems));
    WMAR_TRY(e->mem.alloc(&e->gtmp, e->max_elems));
    WMAR_TRY(e->mem.alloc(&e->ups, e->ups_elems));
    WMAR_TRY(e->mem.alloc(&e->ws, e->ws_elems));
    WMAR_TRY(e->mem.alloc(&e->gnb, e->gnb_doubles));
    WMAR_TRY(e->mem.alloc(&e->dp, e->attn_nn));
    WMAR_TRY(e->mem.alloc(&e->tr, e->attn_nn));
    WMAR_TRY(e->mem.alloc(&e->attk, e->attn_nc * 3 / 8 + 1));
    WMAR_TRY(e->mem.alloc(&e->attv, e->attn_nc * 3 / 8 + 1));
    WMAR_TRY(e->mem.alloc_zero(&e->zbias, zbias_elems, st));
    WMAR_TRY(e->mem.alloc(&e->gn_partial, (size_t)GN_MR_DOUBLES + (size_t)e->Bmax * GN_CHUNKS_MAX * 32 * 2));
    e->gn_tiles_cap = (long long)e->Bmax * (e->cfg.resolution / 8) * (e->cfg.resolution / 8) * 64;
    WMAR_TRY(e->mem.alloc(&e->gn_tiles, (size_t)e->gn_tiles_cap));
}

int train_forward(wmar_vq_train* e, THalf& h, int B, hipStream_t st) {
    int rc;
    g_trk = GnTrack{};
    g_trk.part = e->gn_tiles; g_trk.cap = e->gn_tiles_cap;
    GnRef gn{};
    for (const TOp& o : h.ops) {
        if (o.kind == T_GN) {
            const TTensor& x = e->t[o.in];
            TNorm& n = e->norms[o.norm];
            if ((rc = run_gn(e->gn_partial, n.n, x.d, B, x.H * x.H, o.swish, st, &gn))) return rc;
            WMAR_HIP_CHECK(hipMemcpyAsync(n.mr, gn.mr, (size_t)B * 32 * sizeof(float2), hipMemcpyDeviceToDevice, st));
        } else if (o.kind == T_CONV) {
            const TTensor& x = e->t[o.in];
            if ((rc = run_conv(e->convs[o.conv].fw, x.d, e->t[o.out].d, o.res >= 0 ? e->t[o.res].d : nullptr, B, x.H, x.H, e->convs[o.conv].stride,
                               o.up, st, o.norm >= 0 ? &gn : nullptr))) return rc;
        } else if (o.kind == T_POOL) {                          // wmar_mvq_encode's launch
            const TTensor& x = e->t[o.in];
            const TTensor& y = e->t[o.out];
            const long long total = (long long)y.H * y.H * (x.C / 4);
            int gx = (int)((total + 255) / 256);
            if (gx > 8192) gx = 8192;
            hipLaunchKernelGGL(k_avgpool2, dim3(gx, (unsigned)B), dim3(256), 0, st, (const float*)x.d, y.d, y.H, y.H, x.C);
            if (g_trk.src == y.d) g_trk.src = nullptr;
            if ((rc = launch_status("k_avgpool2"))) return rc;
        } else {
            const TTensor& q = e->t[o.q];
            if ((rc = attn_core(AttnScratch{o.P, e->attk, e->attv, e->zbias}, q.d, e->t[o.k].d, e->t[o.v].d, e->t[o.out].d, B, q.H, q.H, q.C, st)))
                return rc;
        }
    }
    g_trk = GnTrack{};
    return WMAR_OK;
}

// where the next contribution to a tensor's gradient is written, and what to do once it is there
float* grad_target(wmar_vq_train* e, TTensor& x) { return x.gset ? e->gtmp : x.g; }
int grad_commit(wmar_vq_train* e, TTensor& x, int B, hipStream_t st) {
    if (x.gset) {
        const long long n4 = (long long)(x.elems(B) / 4);
        hipLaunchKernelGGL(k_add_into, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, x.g, (const float*)e->gtmp, n4);
        return launch_status("k_add_into");
    }
    x.gset = true;
    return WMAR_OK;
}

// want_input_grad: whether the gradient of the half's first tensor is needed
int train_backward(wmar_vq_train* e, THalf& h, int B, bool want_input_grad, hipStream_t st) {
    int rc;
    g_trk = GnTrack{};
    e->ngy_set = false;
    for (int i = (int)h.ops.size() - 1; i >= 0; --i) {
        const TOp& o = h.ops[i];
        if (o.kind == T_CONV) {
            TConv& c = e->convs[o.conv];
            TTensor& x = e->t[o.in];
            const TTensor& y = e->t[o.out];
            WMAR_REQUIRE(y.gset, "vq_train backward: no gradient reached the output of %s", c.name.c_str());
            if (o.res >= 0) {                                   // the residual passes the gradient through
                TTensor& r = e->t[o.res];
                if (r.gset) {
                    const long long n4 = (long long)(r.elems(B) / 4);
                    hipLaunchKernelGGL(k_add_into, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, r.g, (const float*)y.g, n4);
                } else {
                    WMAR_HIP_CHECK(hipMemcpyAsync(r.g, y.g, r.elems(B) * 4, hipMemcpyDeviceToDevice, st));
                    r.gset = true;
                }
            }
            const float* yin = x.d;                             // the conv's actual input
            if (o.norm >= 0) {
                const TNorm& n = e->norms[o.norm];
                const long long total4 = (long long)(x.elems(B) / 4);
                hipLaunchKernelGGL(k_gn_apply, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, (const float*)x.d, e->ybuf, (const float2*)n.mr,
                                   (const float*)n.n.g, (const float*)n.n.b, total4, x.H * x.H, x.C, o.swish);
                yin = e->ybuf;
            }
            if ((rc = run_conv_wgrad(y.g, yin, c.gw, c.gb, e->ws, c.cout, c.cin, c.ks, B, x.H, x.H, c.stride, o.up, st))) return rc;
            if (o.in == h.first && !want_input_grad) continue;
            if (o.norm >= 0) {                                   // gradient of the normalised activation: the norm's backward runs at its T_GN
                float* dst = e->ngy_set ? e->gtmp : e->ngy;
                if ((rc = run_conv_dgrad(&c.dg, c.w, c.cout, c.cin, c.ks, y.g, dst, e->ups, B, x.H, x.H, c.stride, o.up, st))) return rc;
                if (e->ngy_set) {
                    const long long n4 = (long long)(x.elems(B) / 4);
                    hipLaunchKernelGGL(k_add_into, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, e->ngy, (const float*)e->gtmp, n4);
                }
                e->ngy_set = true;
            } else {
                if ((rc = run_conv_dgrad(c.stride == 1 ? &c.dg : nullptr, c.w, c.cout, c.cin, c.ks, y.g, grad_target(e, x), e->ups, B, x.H, x.H,
                                         c.stride, o.up, st))) return rc;
                if ((rc = grad_commit(e, x, B, st))) return rc;
            }
        } else if (o.kind == T_GN) {
            TTensor& x = e->t[o.in];
            TNorm& n = e->norms[o.norm];
            if (!e->ngy_set) continue;                          // its convs' input gradients were not wanted
            if ((rc = run_gn_backward(x.d, e->ngy, n.mr, n.n.g, n.n.b, n.n.C, B, x.H * x.H, o.swish, e->gnb, grad_target(e, x), n.dg, n.db, st))) return rc;
            if ((rc = grad_commit(e, x, B, st))) return rc;
            e->ngy_set = false;
        } else if (o.kind == T_POOL) {
            TTensor& x = e->t[o.in];
            const TTensor& y = e->t[o.out];
            WMAR_REQUIRE(y.gset, "vq_train backward: no gradient reached the output of an average pool");
            if ((rc = run_avgpool_backward(y.g, grad_target(e, x), B, y.H, y.H, x.C, st))) return rc;
            if ((rc = grad_commit(e, x, B, st))) return rc;
        } else {
            const TTensor& out = e->t[o.out];
            TTensor &q = e->t[o.q], &k = e->t[o.k], &v = e->t[o.v];
            WMAR_REQUIRE(out.gset, "vq_train backward: no gradient reached an attention output");
            if ((rc = attn_backward(AttnScratch{nullptr, e->attk, e->attv, e->zbias}, e->dp, e->tr, q.d, k.d, v.d, o.P, out.g, q.g, k.g, v.g, B, q.H, q.H,
                                    q.C, st))) return rc;
            q.gset = k.gset = v.gset = true;
        }
    }
    return launch_status("vq_train backward");
}

void train_clear_grads(wmar_vq_train* e, THalf& h) {
    for (const TOp& o : h.ops) {
        if (o.in >= 0) e->t[o.in].gset = false;
        if (o.out >= 0) e->t[o.out].gset = false;
    }
}

}  // namespace

extern "C" {

int wmar_vq_train_create(const wmar_vq_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream,
                         wmar_vq_train** out) {
    WMAR_REQUIRE(cfg && names && tensors_dev && out, "vq_train_create: null argument");
    WMAR_REQUIRE(cfg->n_levels >= 1 && cfg->n_levels <= 8, "vq_train_create: bad ch_mult length");
    WMAR_REQUIRE(cfg->max_batch >= 1, "vq_train_create: max_batch");
    WMAR_REQUIRE(cfg->embed_dim % 8 == 0, "embed_dim %% 8 must be 0");
    WMAR_REQUIRE(cfg->ch % 32 == 0, "ch must be a multiple of 32 (GroupNorm has 32 groups)");
    const int L = cfg->n_levels;
    const int S = cfg->resolution >> (L - 1);
    WMAR_REQUIRE(S >= 8 && S % 8 == 0 && (S << (L - 1)) == cfg->resolution, "latent size %d must be a multiple of 8", S);
    auto* e = new wmar_vq_train();
    e->cfg = *cfg; e->Bmax = cfg->max_batch; e->S = S;
    hipStream_t st = (hipStream_t)stream;
    Loader ld(names, tensors_dev, n_tensors, &e->mem, st);
    int& rc = ld.rc;
    TrainBuilder b{e, ld, st, rc};
    const int ch = cfg->ch, z = cfg->z_channels, E = cfg->embed_dim;

    // ---- encoder + quant_conv, in wmar_vq_encode's order
    {
        THalf& h = e->half[0];
        int res = cfg->resolution;
        int x = b.tensor(cfg->in_channels, res);
        h.first = x;
        x = b.op_conv(h, 0, "encoder.conv_in", cfg->in_channels, ch, 3, x, -1, -1, 0, 1, 0);
        int block_in = ch;
        for (int lvl = 0; lvl < L; ++lvl) {
            block_in = ch * (lvl == 0 ? 1 : cfg->ch_mult[lvl - 1]);
            const int block_out = ch * cfg->ch_mult[lvl];
            for (int i = 0; i < cfg->num_res_blocks; ++i) {
                const std::string p = "encoder.down." + std::to_string(lvl) + ".";
                x = b.res(h, 0, p + "block." + std::to_string(i) + ".", block_in, block_out, x);
                block_in = block_out;
                if (in_attn_res(*cfg, res)) x = b.attn(h, 0, p + "attn." + std::to_string(i) + ".", block_in, x);
            }
            if (lvl != L - 1) {
                x = b.op_conv(h, 0, "encoder.down." + std::to_string(lvl) + ".downsample.conv", block_in, block_in, 3, x, -1, -1, 0, 2, 0);
                res /= 2;
            }
        }
        x = b.res(h, 0, "encoder.mid.block_1.", block_in, block_in, x);
        x = b.attn(h, 0, "encoder.mid.attn_1.", block_in, x);
        x = b.res(h, 0, "encoder.mid.block_2.", block_in, block_in, x);
        const int no = b.norm("encoder.norm_out", block_in, 0);
        b.note_norm(block_in, S);
        b.op_gn(h, x, no, 1);
        x = b.op_conv(h, 0, "encoder.conv_out", block_in, z, 3, x, -1, no, 1, 1, 0);
        x = b.op_conv(h, 0, "quant_conv", z, E, 1, x, -1, -1, 0, 1, 0);
        h.last = x;
    }
    // ---- post_quant_conv + decoder, in wmar_vq_decode's order
    {
        THalf& h = e->half[1];
        int block_in = ch * cfg->ch_mult[L - 1];
        int res = S;
        int x = b.tensor(E, S);
        h.first = x;
        x = b.op_conv(h, 1, "post_quant_conv", E, z, 1, x, -1, -1, 0, 1, 0);
        x = b.op_conv(h, 1, "decoder.conv_in", z, block_in, 3, x, -1, -1, 0, 1, 0);
        x = b.res(h, 1, "decoder.mid.block_1.", block_in, block_in, x);
        x = b.attn(h, 1, "decoder.mid.attn_1.", block_in, x);
        x = b.res(h, 1, "decoder.mid.block_2.", block_in, block_in, x);
        for (int lvl = L - 1; lvl >= 0; --lvl) {
            const int block_out = ch * cfg->ch_mult[lvl];
            for (int i = 0; i <= cfg->num_res_blocks; ++i) {
                const std::string p = "decoder.up." + std::to_string(lvl) + ".";
                x = b.res(h, 1, p + "block." + std::to_string(i) + ".", block_in, block_out, x);
                block_in = block_out;
                if (in_attn_res(*cfg, res)) x = b.attn(h, 1, p + "attn." + std::to_string(i) + ".", block_in, x);
            }
            if (lvl != 0) {
                x = b.op_conv(h, 1, "decoder.up." + std::to_string(lvl) + ".upsample.conv", block_in, block_in, 3, x, -1, -1, 0, 1, 1);
                res *= 2;
            }
        }
        const int no = b.norm("decoder.norm_out", block_in, 1);
        b.note_norm(block_in, cfg->resolution);
        b.op_gn(h, x, no, 1);
        x = b.op_conv(h, 1, "decoder.conv_out", block_in, cfg->out_ch, 3, x, -1, no, 1, 1, 0);
        h.last = x;
    }
    {
        int amax = S;
        for (int i = 0; i < cfg->n_attn_res; ++i) amax = cfg->attn_resolutions[i] > amax ? cfg->attn_resolutions[i] : amax;
        int cam = 0;
        for (int lvl = 0; lvl < L; ++lvl) cam = ch * cfg->ch_mult[lvl] > cam ? ch * cfg->ch_mult[lvl] : cam;
        train_scratch(e, rc, (size_t)amax * amax > (size_t)cam ? (size_t)amax * amax : (size_t)cam, st);
    }
    if (rc == WMAR_OK && hipStreamSynchronize(st) != hipSuccess) { set_error("vq_train_create: sync failed"); rc = WMAR_EHIP; }
    if (rc != WMAR_OK) { const int r = rc; delete e; return r; }
    *out = e;
    return WMAR_OK;
}

// The MaskGIT-VQGAN plan (RAR's tokenizer) through the same machinery, written in the order wmar_mvq_encode / wmar_mvq_decode make their
// calls.  Reference: deps/rar/modeling/modules/maskgit_vqgan.py and titok.py:91-208 (decode_like_taming, encode_like_taming_prequant).
int wmar_mvq_train_create(const wmar_mvq_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream,
                          wmar_vq_train** out) {
    WMAR_REQUIRE(cfg && names && tensors_dev && out, "mvq_train_create: null argument");
    WMAR_REQUIRE(cfg->n_levels >= 1 && cfg->n_levels <= 8 && cfg->max_batch >= 1, "mvq_train_create: bad config");
    WMAR_REQUIRE(cfg->z_channels % 8 == 0 && cfg->hidden_channels % 32 == 0, "z_channels %% 8 and hidden_channels %% 32 must be 0");
    const int R = cfg->n_levels, hc = cfg->hidden_channels, z = cfg->z_channels;
    const int S = cfg->resolution >> (R - 1);
    WMAR_REQUIRE(S >= 8 && S % 8 == 0 && (S << (R - 1)) == cfg->resolution, "latent size %d must be a multiple of 8", S);
    auto* e = new wmar_vq_train();
    e->mvq = true; e->Bmax = cfg->max_batch; e->S = S;
    e->cfg.ch = hc; e->cfg.num_res_blocks = cfg->num_res_blocks; e->cfg.resolution = cfg->resolution;
    e->cfg.in_channels = e->cfg.out_ch = cfg->num_channels; e->cfg.z_channels = e->cfg.embed_dim = z;
    e->cfg.n_embed = cfg->num_embeddings; e->cfg.n_levels = R; e->cfg.max_batch = cfg->max_batch;
    for (int i = 0; i < R; ++i) e->cfg.ch_mult[i] = cfg->channel_mult[i];
    hipStream_t st = (hipStream_t)stream;
    Loader ld(names, tensors_dev, n_tensors, &e->mem, st);
    int& rc = ld.rc;
    TrainBuilder b{e, ld, st, rc};
    const int mid = hc * cfg->channel_mult[R - 1];
    // ---- encoder, in wmar_mvq_encode's order
    {
        THalf& h = e->half[0];
        int x = b.tensor(cfg->num_channels, cfg->resolution);
        h.first = x;
        x = b.op_conv(h, 0, "encoder.conv_in", cfg->num_channels, hc, 3, x, -1, -1, 0, 1, 0, false);
        for (int lvl = 0; lvl < R; ++lvl) {
            int bi = hc * (lvl == 0 ? 1 : cfg->channel_mult[lvl - 1]);
            const int bo = hc * cfg->channel_mult[lvl];
            for (int i = 0; i < cfg->num_res_blocks; ++i) {
                x = b.mres(h, 0, "encoder.down." + std::to_string(lvl) + ".block." + std::to_string(i) + ".", bi, bo, x);
                bi = bo;
            }
            if (lvl != R - 1) x = b.op_pool(h, x);
        }
        for (int i = 0; i < cfg->num_res_blocks; ++i) x = b.mres(h, 0, "encoder.mid." + std::to_string(i) + ".", mid, mid, x);
        const int no = b.norm("encoder.norm_out", mid, 0);
        b.note_norm(mid, S);
        b.op_gn(h, x, no, 1);
        h.last = b.op_conv(h, 0, "encoder.conv_out", mid, z, 1, x, -1, no, 1, 1, 0);
    }
    // ---- decoder, in wmar_mvq_decode's order
    {
        THalf& h = e->half[1];
        int x = b.tensor(z, S);
        h.first = x;
        x = b.op_conv(h, 1, "decoder.conv_in", z, mid, 3, x, -1, -1, 0, 1, 0);
        for (int i = 0; i < cfg->num_res_blocks; ++i) x = b.mres(h, 1, "decoder.mid." + std::to_string(i) + ".", mid, mid, x);
        for (int lvl = R - 1; lvl >= 0; --lvl) {
            int bi = lvl == R - 1 ? mid : hc * cfg->channel_mult[lvl + 1];
            const int bo = hc * cfg->channel_mult[lvl];
            for (int i = 0; i < cfg->num_res_blocks; ++i) {
                x = b.mres(h, 1, "decoder.up." + std::to_string(lvl) + ".block." + std::to_string(i) + ".", bi, bo, x);
                bi = bo;
            }
            if (lvl != 0) x = b.op_conv(h, 1, "decoder.up." + std::to_string(lvl) + ".upsample_conv", bo, bo, 3, x, -1, -1, 0, 1, 1);
        }
        const int no = b.norm("decoder.norm_out", hc * cfg->channel_mult[0], 1);
        b.note_norm(hc * cfg->channel_mult[0], cfg->resolution);
        b.op_gn(h, x, no, 1);
        h.last = b.op_conv(h, 1, "decoder.conv_out", hc * cfg->channel_mult[0], cfg->num_channels, 3, x, -1, no, 1, 1, 0);
    }
    train_scratch(e, rc, 1, st);                               // no attention in this network
    if (rc == WMAR_OK && hipStreamSynchronize(st) != hipSuccess) { set_error("mvq_train_create: sync failed"); rc = WMAR_EHIP; }
    if (rc != WMAR_OK) { const int r = rc; delete e; return r; }
    *out = e;
    return WMAR_OK;
}

void wmar_vq_train_destroy(wmar_vq_train* e) { delete e; }
int64_t wmar_vq_train_device_bytes(const wmar_vq_train* e) { return e ? e->mem.bytes : 0; }

int wmar_vq_train_set_weights(wmar_vq_train* e, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream) {
    WMAR_REQUIRE(e && names && tensors_dev, "vq_train_set_weights: null argument");
    hipStream_t st = (hipStream_t)stream;
    TensorMap tm(names, tensors_dev, n_tensors);
    // every name is looked up before anything is written
    for (const TConv& c : e->convs) { (void)(const float*)tm.need(c.name + ".weight"); if (c.bias) (void)(const float*)tm.need(c.name + ".bias"); }
    for (const TNorm& n : e->norms) { (void)(const float*)tm.need(n.name + ".weight"); (void)(const float*)tm.need(n.name + ".bias"); }
    if (tm.rc) return tm.rc;
    e->half[0].tape = e->half[1].tape = false;
    for (TConv& c : e->convs)
        if (int rc = repack_conv(c, tm.get(c.name + ".weight"), c.bias ? (const float*)tm.get(c.name + ".bias") : nullptr, st)) return rc;
    for (TNorm& n : e->norms) {
        WMAR_HIP_CHECK(hipMemcpyAsync(n.n.g, tm.get(n.name + ".weight"), (size_t)n.n.C * 4, hipMemcpyDeviceToDevice, st));
        WMAR_HIP_CHECK(hipMemcpyAsync(n.n.b, tm.get(n.name + ".bias"), (size_t)n.n.C * 4, hipMemcpyDeviceToDevice, st));
    }
    return WMAR_OK;
}

int wmar_vq_train_encode(wmar_vq_train* e, const float* images_dev, int64_t B, float* prequant_dev, void* stream) {
    WMAR_REQUIRE(e && images_dev && prequant_dev, "vq_train_encode: null argument");
    WMAR_REQUIRE(B >= 1 && B <= e->Bmax, "vq_train_encode: batch %lld outside 1..%d", (long long)B, e->Bmax);
    hipStream_t st = (hipStream_t)stream;
    THalf& h = e->half[0];
    h.tape = false; h.grads = false;
    const int R = e->cfg.resolution;
    const TTensor& x0 = e->t[h.first];
    hipLaunchKernelGGL(e->mvq ? k_nchw_to_nhwc01 : k_nchw_to_nhwc, dim3((R * R + 255) / 256, (unsigned)B), dim3(256), 0, st, images_dev, x0.d,
                       e->cfg.in_channels, R * R, x0.C);
    if (int rc = launch_status("k_nchw_to_nhwc")) return rc;
    if (int rc = train_forward(e, h, (int)B, st)) return rc;
    const TTensor& zo = e->t[h.last];
    WMAR_HIP_CHECK(hipMemcpyAsync(prequant_dev, zo.d, zo.elems((int)B) * 4, hipMemcpyDeviceToDevice, st));
    h.tape = true; h.B = (int)B;
    return WMAR_OK;
}

int wmar_vq_train_encode_backward(wmar_vq_train* e, const float* grad_prequant_dev, int64_t B, float* grad_images_dev, void* stream) {
    WMAR_REQUIRE(e && grad_prequant_dev, "vq_train_encode_backward: null argument");
    THalf& h = e->half[0];
    WMAR_REQUIRE(h.tape, "vq_train_encode_backward: no tape (no wmar_vq_train_encode since create or the last wmar_vq_train_set_weights)");
    WMAR_REQUIRE(B == h.B, "vq_train_encode_backward: batch %lld, the tape holds %d", (long long)B, h.B);
    hipStream_t st = (hipStream_t)stream;
    h.grads = false;
    train_clear_grads(e, h);
    TTensor& zo = e->t[h.last];
    WMAR_HIP_CHECK(hipMemcpyAsync(zo.g, grad_prequant_dev, zo.elems((int)B) * 4, hipMemcpyDeviceToDevice, st));
    zo.gset = true;
    if (int rc = train_backward(e, h, (int)B, grad_images_dev != nullptr, st)) return rc;
    if (grad_images_dev) {
        const int R = e->cfg.resolution;
        const TTensor& x0 = e->t[h.first];
        if (e->mvq) {                                           // through (x + 1) / 2
            if (int rc = run_mvq_input_backward(x0.g, grad_images_dev, (int)B, e->cfg.in_channels, R * R, x0.C, st)) return rc;
        } else {
            hipLaunchKernelGGL(k_nhwc_to_nchw, dim3((R * R + 255) / 256, (unsigned)B), dim3(256), 0, st, (const float*)x0.g, grad_images_dev,
                               e->cfg.in_channels, R * R, x0.C);
            if (int rc = launch_status("k_nhwc_to_nchw")) return rc;
        }
    }
    h.grads = true;
    return WMAR_OK;
}

int wmar_vq_train_decode(wmar_vq_train* e, const float* zq_dev, int64_t B, float* images_dev, void* stream) {
    WMAR_REQUIRE(e && zq_dev && images_dev, "vq_train_decode: null argument");
    WMAR_REQUIRE(B >= 1 && B <= e->Bmax, "vq_train_decode: batch %lld outside 1..%d", (long long)B, e->Bmax);
    hipStream_t st = (hipStream_t)stream;
    THalf& h = e->half[1];
    h.tape = false; h.grads = false;
    const TTensor& x0 = e->t[h.first];
    WMAR_HIP_CHECK(hipMemcpyAsync(x0.d, zq_dev, x0.elems((int)B) * 4, hipMemcpyDeviceToDevice, st));
    if (int rc = train_forward(e, h, (int)B, st)) return rc;
    const int R = e->cfg.resolution;
    const TTensor& yo = e->t[h.last];
    hipLaunchKernelGGL(e->mvq ? k_nhwc_to_nchw_01 : k_nhwc_to_nchw, dim3((R * R + 255) / 256, (unsigned)B), dim3(256), 0, st, (const float*)yo.d,
                       images_dev, e->cfg.out_ch, R * R, yo.C);
    if (int rc = launch_status("k_nhwc_to_nchw")) return rc;
    h.tape = true; h.B = (int)B;
    return WMAR_OK;
}

int wmar_vq_train_decode_backward(wmar_vq_train* e, const float* grad_images_dev, int64_t B, float* grad_zq_dev, void* stream) {
    WMAR_REQUIRE(e && grad_images_dev, "vq_train_decode_backward: null argument");
    THalf& h = e->half[1];
    WMAR_REQUIRE(h.tape, "vq_train_decode_backward: no tape (no wmar_vq_train_decode since create or the last wmar_vq_train_set_weights)");
    WMAR_REQUIRE(B == h.B, "vq_train_decode_backward: batch %lld, the tape holds %d", (long long)B, h.B);
    hipStream_t st = (hipStream_t)stream;
    h.grads = false;
    train_clear_grads(e, h);
    const int R = e->cfg.resolution;
    TTensor& yo = e->t[h.last];
    if (e->mvq) {                                               // through clamp(v, 0, 1) * 2 - 1 on the taped v
        if (int rc = run_mvq_image_backward(yo.d, grad_images_dev, yo.g, (int)B, e->cfg.out_ch, R * R, yo.C, st)) return rc;
    } else {
        hipLaunchKernelGGL(k_nchw_to_nhwc, dim3((R * R + 255) / 256, (unsigned)B), dim3(256), 0, st, grad_images_dev, yo.g, e->cfg.out_ch, R * R, yo.C);
        if (int rc = launch_status("k_nchw_to_nhwc")) return rc;
    }
    yo.gset = true;
    if (int rc = train_backward(e, h, (int)B, grad_zq_dev != nullptr, st)) return rc;
    if (grad_zq_dev) {
        const TTensor& x0 = e->t[h.first];
        WMAR_HIP_CHECK(hipMemcpyAsync(grad_zq_dev, x0.g, x0.elems((int)B) * 4, hipMemcpyDeviceToDevice, st));
    }
    h.grads = true;
    return WMAR_OK;
}

int wmar_vq_train_get_grads(wmar_vq_train* e, const char* const* names, void* const* grads_dev, int32_t n, int32_t accumulate, void* stream) {
    WMAR_REQUIRE(e && names && grads_dev, "vq_train_get_grads: null argument");
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < n; ++i) {
        WMAR_REQUIRE(names[i] && grads_dev[i], "vq_train_get_grads: null entry %d", i);
        auto it = e->grad_of.find(names[i]);
        WMAR_REQUIRE(it != e->grad_of.end(), "vq_train_get_grads: '%s' is not a trainable tensor", names[i]);
        WMAR_REQUIRE(e->half[it->second.half].grads, "vq_train_get_grads: '%s': its half has run no backward", names[i]);
    }
    for (int i = 0; i < n; ++i) {
        const TGrad& g = e->grad_of[names[i]];
        if (accumulate) {
            hipLaunchKernelGGL(k_add_into1, dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, st, (float*)grads_dev[i], (const float*)g.p, (long long)g.n);
        } else {
            WMAR_HIP_CHECK(hipMemcpyAsync(grads_dev[i], g.p, g.n * 4, hipMemcpyDeviceToDevice, st));
        }
    }
    return launch_status("vq_train_get_grads");
}

}  // extern "C"
