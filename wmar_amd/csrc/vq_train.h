// Trainable VQGAN tokenizers (gfx950; Taming and RAR's MaskGIT-VQGAN): a forward that records a tape, and the backward of encoder + quant_conv
// and of post_quant_conv + decoder, built from the layer functions of vq_grad.h.  Included at the end of vqgan.hip behind vq_grad.h.
//
// Reference: deps/taming/models/vqgan.py:64-73 (encode / decode) under torch.autograd, as finetune.py trains them
// (deps/taming/models/vqgan.py:86-169); deps/rar/modeling/titok.py:91-208 (decode_like_taming, encode_like_taming_prequant).  Dropout is 0
// and GroupNorm has no train mode: the training forward IS the inference forward.
//
// The network is the plan the inference engine executes (vq_plan.h) and the forward is the same executor (vq_forward in vqgan.hip), so a
// training forward launches the same kernels on the same values and is bit-equal to inference.  What differs is where results go: every
// tensor has memory of its own (the tape) instead of a slot buffer, every norm's (mean, rstd) is copied out of the shared table, every
// attention keeps its softmax.  The backward walks the op list in reverse.  A gradient buffer that already holds a contribution (the input
// of a ResnetBlock: shortcut + norm1 path; the input of an AttnBlock: residual + q, k, v) gets the next one through a scratch buffer and
// an elementwise add -- stream order, no atomics.  The convs behind one norm (q, k, v) add their input gradients into one buffer first;
// the norm's backward then runs once.  All memory is allocated at create time for max_batch images.
//
// For the MaskGIT-VQGAN plan the [-1, 1] <-> [0, 1] range change and the clamp are differentiated at the image edges.
//
// A FROZEN handle (wmar_vq_train_create_frozen / wmar_mvq_train_create_frozen) is the forward alone: the same packed weights and the same
// executor, with the tensors in the plan's slot buffers as the inference engines have them (tensor i at slot[p.t[i].slot]) and no tape
// passed -- nothing of the backward is allocated, and the backward entries refuse the handle.  set_weights repacks from the caller's
// tensors directly.
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

// what the tape and the backward add to the plan's tensors, norms and convs (same indices)
struct TTensor : VqTensor { float* d = nullptr; float* g = nullptr; bool gset = false; };
struct TNorm { float *dg = nullptr, *db = nullptr; };
struct TConv {
    ConvW dg;                           // the flipped, transposed weights of a stride-1 conv, packed as the forward's are
    float *w = nullptr, *wt = nullptr;  // raw weight (the stride-2 gather reads it), flipped weight
    float *gw = nullptr, *gb = nullptr; // gb stays null for a bias-free conv: no ".bias" gradient
};
struct THalf { int B = 0; bool tape = false, grads = false; };
struct TGrad { float* p; size_t n; int half; };

}  // namespace

struct wmar_vq_train {
    DeviceArena mem;
    VqNet net;                          // net.at[i] == t[i].d
    VqTape tape;
    std::vector<TTensor> t;
    std::vector<TNorm> norms;
    std::vector<TConv> convs;
    THalf half[2];                      // 0 = encoder + quant_conv, 1 = post_quant_conv + decoder
    std::map<std::string, TGrad> grad_of;
    // scratch of the backward
    double* gnb = nullptr;
    float *ybuf = nullptr, *ngy = nullptr, *gtmp = nullptr, *ups = nullptr, *ws = nullptr, *dp = nullptr, *tr = nullptr;
    bool ngy_set = false;
    bool frozen = false;                // forward only: t[i].d are slot buffers, t[i].g and everything the backward reads are null
};

namespace {

// (re)pack a conv's forward and dgrad weights from a torch-layout weight and bias: Loader::conv without the allocations
int repack_conv(const VqConvDesc& d, ConvW& fw, TConv& c, const float* W, const float* bias, hipStream_t st) {
    auto pack = [&](ConvW& p, const float* src, int cin, int cout, const float* b) {
        const int T = d.ks * d.ks;
        const size_t n = (size_t)p.CT * T * p.KBc * 64;
        hipLaunchKernelGGL(k_pack_conv, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, p.wp, cout, cin, d.ks, p.CT, p.KBc);
        if (b) hipLaunchKernelGGL(k_pad_vec, dim3((p.CT * 32 + 255) / 256), dim3(256), 0, st, b, p.bias, cout, p.CT * 32);
        if (p.wq) {
            const size_t nq = (size_t)p.CT * T * (p.cin_s / 16) * 64;
            hipLaunchKernelGGL(k_pack_conv_bx, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, src, p.wq, cout, cin, d.ks, p.CT, p.cin_s / 16);
        }
        if (p.wf) {
            const size_t nf = (size_t)p.cin_s * 9 * 4;
            hipLaunchKernelGGL(k_pack_conv_few, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, src, p.wf, cout, cin, p.cin_s);
        }
    };
    const size_t nw = (size_t)d.cout * d.cin * d.ks * d.ks;
    if (!c.w) {                                         // a frozen handle keeps no raw copy and no dgrad pack
        pack(fw, W, d.cin, d.cout, bias);
        return launch_status("repack_conv");
    }
    WMAR_HIP_CHECK(hipMemcpyAsync(c.w, W, nw * 4, hipMemcpyDeviceToDevice, st));
    pack(fw, c.w, d.cin, d.cout, bias);
    if (d.stride == 1) {
        hipLaunchKernelGGL(k_flip_transpose_w, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, (const float*)c.w, c.wt, d.cout, d.cin, d.ks);
        pack(c.dg, c.wt, d.cout, d.cin, nullptr);      // zero bias stays zero
    }
    return launch_status("repack_conv");
}

// A plan as a training handle: the weights, the tape (every tensor's value and gradient, every norm's statistics, every attention's
// softmax), what the backward needs of every conv and norm, and the backward's scratch sized by the largest layer.
int train_create(VqPlan plan, const char* who, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream,
                 wmar_vq_train** out, bool frozen = false) {
    WMAR_REQUIRE(names && tensors_dev && out, "%s: null argument", who);
    WMAR_REQUIRE(plan.err.empty(), "%s", plan.err.c_str());
    std::unique_ptr<wmar_vq_train> e(new wmar_vq_train());
    e->net.plan = std::move(plan);
    const VqPlan& p = e->net.plan;
    const int Bmax = p.max_batch;
    hipStream_t st = (hipStream_t)stream;
    Loader ld(names, tensors_dev, n_tensors, &e->mem, st);
    int& rc = ld.rc;
    net_load(e->net, ld);
    e->frozen = frozen;
    if (frozen) {                       // one buffer per slot, as large as the largest tensor the plan puts there (engine_create, vqgan.hip)
        float* slot[VQ_SLOTS] = {};
        for (int s = 0; s < VQ_SLOTS; ++s)
            if (s < 4 || p.att_elems) WMAR_TRY(e->mem.alloc(&slot[s], (size_t)Bmax * (s < 4 ? p.rot_elems : p.att_elems)));
        for (const VqTensor& pt : p.t) {
            TTensor tt; static_cast<VqTensor&>(tt) = pt;
            tt.d = slot[pt.slot];
            e->t.push_back(tt);
            e->net.at.push_back(tt.d);
        }
        e->norms.resize(p.norms.size()); e->convs.resize(p.convs.size());
        if (p.attn_nn) WMAR_TRY(e->mem.alloc(&e->net.att.asc, (size_t)Bmax * p.attn_nn));
        net_scratch(e->net, e->mem, rc, st);
        if (rc == WMAR_OK && hipStreamSynchronize(st) != hipSuccess) { set_error("%s: sync failed", who); rc = WMAR_EHIP; }
        if (rc != WMAR_OK) return rc;
        *out = e.release();
        return WMAR_OK;
    }
    for (const VqTensor& pt : p.t) {
        TTensor tt; static_cast<VqTensor&>(tt) = pt;
        WMAR_TRY(e->mem.alloc(&tt.d, tt.elems(Bmax)));
        WMAR_TRY(e->mem.alloc(&tt.g, tt.elems(Bmax)));
        e->t.push_back(tt);
        e->net.at.push_back(tt.d);
    }
    e->norms.resize(p.norms.size()); e->convs.resize(p.convs.size());
    e->tape.mr.resize(p.norms.size(), nullptr); e->tape.P.resize(p.t.size(), nullptr);
    size_t ups_elems = 0, ws_elems = 0, gnb_doubles = 0;
    for (int hidx = 0; hidx < 2; ++hidx)
        for (const VqOp& o : p.half[hidx].ops) {
            if (o.kind == VQ_GN) {
                const VqNormDesc& d = p.norms[o.norm];
                TNorm& n = e->norms[o.norm];
                WMAR_TRY(e->mem.alloc(&n.dg, (size_t)d.C));
                WMAR_TRY(e->mem.alloc(&n.db, (size_t)d.C));
                WMAR_TRY(e->mem.alloc(&e->tape.mr[o.norm], (size_t)Bmax * 32));
                e->grad_of[d.name + ".weight"] = TGrad{n.dg, (size_t)d.C, hidx};
                e->grad_of[d.name + ".bias"] = TGrad{n.db, (size_t)d.C, hidx};
                const int H = p.t[o.in].H;
                gnb_doubles = std::max(gnb_doubles, gnb_scratch_doubles(Bmax, H * H, d.C));
            } else if (o.kind == VQ_CONV) {
                const VqConvDesc& d = p.convs[o.conv];
                TConv& c = e->convs[o.conv];
                const size_t nw = (size_t)d.cout * d.cin * d.ks * d.ks;
                const float* W = ld.need(d.name + ".weight");
                WMAR_TRY(e->mem.alloc(&c.w, nw));
                WMAR_TRY(e->mem.alloc(&c.gw, nw));
                if (d.bias) WMAR_TRY(e->mem.alloc(&c.gb, (size_t)d.cout));
                if (rc == WMAR_OK && hipMemcpyAsync(c.w, W, nw * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { set_error("weight copy failed"); rc = WMAR_EHIP; }
                if (d.stride == 1 && rc == WMAR_OK) {
                    WMAR_TRY(e->mem.alloc(&c.wt, nw));
                    if (rc == WMAR_OK) {
                        hipLaunchKernelGGL(k_flip_transpose_w, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, (const float*)c.w, c.wt, d.cout, d.cin, d.ks);
                        const char* dnames[1] = {"dgrad.weight"};
                        const void* dtensors[1] = {c.wt};
                        Loader l2(dnames, dtensors, 1, &e->mem, st);
                        l2.conv("dgrad", d.cout, d.cin, d.ks, c.dg, false);
                        rc = l2.rc;
                    }
                }
                e->grad_of[d.name + ".weight"] = TGrad{c.gw, nw, hidx};
                if (d.bias) e->grad_of[d.name + ".bias"] = TGrad{c.gb, (size_t)d.cout, hidx};
                const int Ho = p.t[o.out].H;
                if (o.up) ups_elems = std::max(ups_elems, (size_t)Bmax * Ho * Ho * pad8(d.cin));
                ws_elems = std::max(ws_elems, wgrad_ws_elems(Bmax * Ho * Ho, d.cout, d.cin, d.ks));
            } else if (o.kind == VQ_ATTN) {
                const size_t N = (size_t)p.t[o.out].H * p.t[o.out].H;
                WMAR_TRY(e->mem.alloc(&e->tape.P[o.out], (size_t)Bmax * N * N));
            }
        }
    WMAR_TRY(e->mem.alloc(&e->ybuf, Bmax * p.max_elems));
    WMAR_TRY(e->mem.alloc(&e->ngy, Bmax * p.max_elems));
    WMAR_TRY(e->mem.alloc(&e->gtmp, Bmax * p.max_elems));
    WMAR_TRY(e->mem.alloc(&e->ups, ups_elems));
    WMAR_TRY(e->mem.alloc(&e->ws, ws_elems));
    WMAR_TRY(e->mem.alloc(&e->gnb, gnb_doubles));
    WMAR_TRY(e->mem.alloc(&e->dp, Bmax * p.attn_nn));
    WMAR_TRY(e->mem.alloc(&e->tr, Bmax * p.attn_nn));
    net_scratch(e->net, e->mem, rc, st);
    if (rc == WMAR_OK && hipStreamSynchronize(st) != hipSuccess) { set_error("%s: sync failed", who); rc = WMAR_EHIP; }
    if (rc != WMAR_OK) return rc;
    *out = e.release();
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
int train_backward(wmar_vq_train* e, const VqHalf& h, int B, bool want_input_grad, hipStream_t st) {
    int rc;
    const VqPlan& p = e->net.plan;
    const AttnScratch& att = e->net.att;
    g_trk = GnTrack{};
    e->ngy_set = false;
    for (int i = (int)h.ops.size() - 1; i >= 0; --i) {
        const VqOp& o = h.ops[i];
        if (o.kind == VQ_CONV) {
            const VqConvDesc& d = p.convs[o.conv];
            TConv& c = e->convs[o.conv];
            TTensor& x = e->t[o.in];
            const TTensor& y = e->t[o.out];
            WMAR_REQUIRE(y.gset, "vq_train backward: no gradient reached the output of %s", d.name.c_str());
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
                const NormW& n = e->net.nw[o.norm];
                const long long total4 = (long long)(x.elems(B) / 4);
                hipLaunchKernelGGL(k_gn_apply, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, (const float*)x.d, e->ybuf,
                                   (const float2*)e->tape.mr[o.norm], (const float*)n.g, (const float*)n.b, total4, x.H * x.H, x.C, o.swish);
                yin = e->ybuf;
            }
            if ((rc = run_conv_wgrad(y.g, yin, c.gw, c.gb, e->ws, d.cout, d.cin, d.ks, B, x.H, x.H, d.stride, o.up, st))) return rc;
            if (o.in == h.first && !want_input_grad) continue;
            if (o.norm >= 0) {                                   // gradient of the normalised activation: the norm's backward runs at its VQ_GN
                float* dst = e->ngy_set ? e->gtmp : e->ngy;
                if ((rc = run_conv_dgrad(&c.dg, c.w, d.cout, d.cin, d.ks, y.g, dst, e->ups, B, x.H, x.H, d.stride, o.up, st))) return rc;
                if (e->ngy_set) {
                    const long long n4 = (long long)(x.elems(B) / 4);
                    hipLaunchKernelGGL(k_add_into, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, e->ngy, (const float*)e->gtmp, n4);
                }
                e->ngy_set = true;
            } else {
                if ((rc = run_conv_dgrad(d.stride == 1 ? &c.dg : nullptr, c.w, d.cout, d.cin, d.ks, y.g, grad_target(e, x), e->ups, B, x.H, x.H,
                                         d.stride, o.up, st))) return rc;
                if ((rc = grad_commit(e, x, B, st))) return rc;
            }
        } else if (o.kind == VQ_GN) {
            TTensor& x = e->t[o.in];
            const NormW& n = e->net.nw[o.norm];
            if (!e->ngy_set) continue;                          // its convs' input gradients were not wanted
            if ((rc = run_gn_backward(x.d, e->ngy, e->tape.mr[o.norm], n.g, n.b, n.C, B, x.H * x.H, o.swish, e->gnb, grad_target(e, x),
                                      e->norms[o.norm].dg, e->norms[o.norm].db, st))) return rc;
            if ((rc = grad_commit(e, x, B, st))) return rc;
            e->ngy_set = false;
        } else if (o.kind == VQ_POOL) {
            TTensor& x = e->t[o.in];
            const TTensor& y = e->t[o.out];
            WMAR_REQUIRE(y.gset, "vq_train backward: no gradient reached the output of an average pool");
            if ((rc = run_avgpool_backward(y.g, grad_target(e, x), B, y.H, y.H, x.C, st))) return rc;
            if ((rc = grad_commit(e, x, B, st))) return rc;
        } else {
            const TTensor& out = e->t[o.out];
            TTensor &q = e->t[o.q], &k = e->t[o.k], &v = e->t[o.v];
            WMAR_REQUIRE(out.gset, "vq_train backward: no gradient reached an attention output");
            if ((rc = attn_backward(AttnScratch{nullptr, att.attk, att.attv, att.zbias}, e->dp, e->tr, q.d, k.d, v.d, e->tape.P[o.out], out.g, q.g, k.g,
                                    v.g, B, q.H, q.H, q.C, st))) return rc;
            q.gset = k.gset = v.gset = true;
        }
    }
    return launch_status("vq_train backward");
}

void train_clear_grads(wmar_vq_train* e, const VqHalf& h) {
    for (const VqOp& o : h.ops) {
        if (o.in >= 0) e->t[o.in].gset = false;
        if (o.out >= 0) e->t[o.out].gset = false;
    }
}

}  // namespace

extern "C" {

int wmar_vq_train_create(const wmar_vq_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream,
                         wmar_vq_train** out) {
    WMAR_REQUIRE(cfg, "vq_train_create: null argument");
    return train_create(plan_taming(*cfg, "vq_train_create"), "vq_train_create", names, tensors_dev, n_tensors, stream, out);
}

int wmar_mvq_train_create(const wmar_mvq_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream,
                          wmar_vq_train** out) {
    WMAR_REQUIRE(cfg, "mvq_train_create: null argument");
    return train_create(plan_mvq(*cfg, "mvq_train_create"), "mvq_train_create", names, tensors_dev, n_tensors, stream, out);
}

int wmar_vq_train_create_frozen(const wmar_vq_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors,
                                void* stream, wmar_vq_train** out) {
    WMAR_REQUIRE(cfg, "vq_train_create_frozen: null argument");
    return train_create(plan_taming(*cfg, "vq_train_create_frozen"), "vq_train_create_frozen", names, tensors_dev, n_tensors, stream, out, true);
}

int wmar_mvq_train_create_frozen(const wmar_mvq_config* cfg, const char* const* names, const void* const* tensors_dev, int32_t n_tensors,
                                 void* stream, wmar_vq_train** out) {
    WMAR_REQUIRE(cfg, "mvq_train_create_frozen: null argument");
    return train_create(plan_mvq(*cfg, "mvq_train_create_frozen"), "mvq_train_create_frozen", names, tensors_dev, n_tensors, stream, out, true);
}

void wmar_vq_train_destroy(wmar_vq_train* e) { delete e; }
int64_t wmar_vq_train_device_bytes(const wmar_vq_train* e) { return e ? e->mem.bytes : 0; }

int wmar_vq_train_set_weights(wmar_vq_train* e, const char* const* names, const void* const* tensors_dev, int32_t n_tensors, void* stream) {
    WMAR_REQUIRE(e && names && tensors_dev, "vq_train_set_weights: null argument");
    hipStream_t st = (hipStream_t)stream;
    const VqPlan& p = e->net.plan;
    TensorMap tm(names, tensors_dev, n_tensors);
    // every name is looked up before anything is written
    for (const VqConvDesc& c : p.convs) { (void)(const float*)tm.need(c.name + ".weight"); if (c.bias) (void)(const float*)tm.need(c.name + ".bias"); }
    for (const VqNormDesc& n : p.norms) { (void)(const float*)tm.need(n.name + ".weight"); (void)(const float*)tm.need(n.name + ".bias"); }
    if (tm.rc) return tm.rc;
    e->half[0].tape = e->half[1].tape = false;
    for (size_t i = 0; i < p.convs.size(); ++i) {
        const VqConvDesc& c = p.convs[i];
        if (int rc = repack_conv(c, e->net.cw[i], e->convs[i], tm.get(c.name + ".weight"), c.bias ? tm.get(c.name + ".bias") : nullptr, st)) return rc;
    }
    for (size_t i = 0; i < p.norms.size(); ++i) {
        const VqNormDesc& n = p.norms[i];
        WMAR_HIP_CHECK(hipMemcpyAsync(e->net.nw[i].g, tm.get(n.name + ".weight"), (size_t)n.C * 4, hipMemcpyDeviceToDevice, st));
        WMAR_HIP_CHECK(hipMemcpyAsync(e->net.nw[i].b, tm.get(n.name + ".bias"), (size_t)n.C * 4, hipMemcpyDeviceToDevice, st));
    }
    return WMAR_OK;
}

int wmar_vq_train_encode(wmar_vq_train* e, const float* images_dev, int64_t B, float* prequant_dev, void* stream) {
    WMAR_REQUIRE(e && images_dev && prequant_dev, "vq_train_encode: null argument");
    const VqPlan& p = e->net.plan;
    WMAR_REQUIRE(B >= 1 && B <= p.max_batch, "vq_train_encode: batch %lld outside 1..%d", (long long)B, p.max_batch);
    hipStream_t st = (hipStream_t)stream;
    THalf& s = e->half[0];
    s.tape = false; s.grads = false;
    const int HW = p.resolution * p.resolution;
    const TTensor& x0 = e->t[p.half[0].first];
    hipLaunchKernelGGL(p.unit_range ? k_nchw_to_nhwc01 : k_nchw_to_nhwc, dim3((HW + 255) / 256, (unsigned)B), dim3(256), 0, st, images_dev, x0.d,
                       p.in_channels, HW, x0.C);
    if (int rc = launch_status("k_nchw_to_nhwc")) return rc;
    if (int rc = vq_forward(e->net, p.half[0], (int)B, st, e->frozen ? nullptr : &e->tape)) return rc;
    const TTensor& zo = e->t[p.half[0].last];
    WMAR_HIP_CHECK(hipMemcpyAsync(prequant_dev, zo.d, zo.elems((int)B) * 4, hipMemcpyDeviceToDevice, st));
    s.tape = !e->frozen; s.B = (int)B;
    return WMAR_OK;
}

int wmar_vq_train_encode_backward(wmar_vq_train* e, const float* grad_prequant_dev, int64_t B, float* grad_images_dev, void* stream) {
    WMAR_REQUIRE(e && grad_prequant_dev, "vq_train_encode_backward: null argument");
    WMAR_REQUIRE(!e->frozen, "vq_train_encode_backward: a frozen handle has no tape and no gradients (wmar_vq_train_create_frozen)");
    const VqPlan& p = e->net.plan;
    const VqHalf& h = p.half[0];
    THalf& s = e->half[0];
    WMAR_REQUIRE(s.tape, "vq_train_encode_backward: no tape (no wmar_vq_train_encode since create or the last wmar_vq_train_set_weights)");
    WMAR_REQUIRE(B == s.B, "vq_train_encode_backward: batch %lld, the tape holds %d", (long long)B, s.B);
    hipStream_t st = (hipStream_t)stream;
    s.grads = false;
    train_clear_grads(e, h);
    TTensor& zo = e->t[h.last];
    WMAR_HIP_CHECK(hipMemcpyAsync(zo.g, grad_prequant_dev, zo.elems((int)B) * 4, hipMemcpyDeviceToDevice, st));
    zo.gset = true;
    if (int rc = train_backward(e, h, (int)B, grad_images_dev != nullptr, st)) return rc;
    if (grad_images_dev) {
        const int HW = p.resolution * p.resolution;
        const TTensor& x0 = e->t[h.first];
        if (p.unit_range) {                                     // through (x + 1) / 2
            if (int rc = run_mvq_input_backward(x0.g, grad_images_dev, (int)B, p.in_channels, HW, x0.C, st)) return rc;
        } else {
            hipLaunchKernelGGL(k_nhwc_to_nchw, dim3((HW + 255) / 256, (unsigned)B), dim3(256), 0, st, (const float*)x0.g, grad_images_dev,
                               p.in_channels, HW, x0.C);
            if (int rc = launch_status("k_nhwc_to_nchw")) return rc;
        }
    }
    s.grads = true;
    return WMAR_OK;
}

int wmar_vq_train_decode(wmar_vq_train* e, const float* zq_dev, int64_t B, float* images_dev, void* stream) {
    WMAR_REQUIRE(e && zq_dev && images_dev, "vq_train_decode: null argument");
    const VqPlan& p = e->net.plan;
    WMAR_REQUIRE(B >= 1 && B <= p.max_batch, "vq_train_decode: batch %lld outside 1..%d", (long long)B, p.max_batch);
    hipStream_t st = (hipStream_t)stream;
    THalf& s = e->half[1];
    s.tape = false; s.grads = false;
    const TTensor& x0 = e->t[p.half[1].first];
    WMAR_HIP_CHECK(hipMemcpyAsync(x0.d, zq_dev, x0.elems((int)B) * 4, hipMemcpyDeviceToDevice, st));
    if (int rc = vq_forward(e->net, p.half[1], (int)B, st, e->frozen ? nullptr : &e->tape)) return rc;
    const int HW = p.resolution * p.resolution;
    const TTensor& yo = e->t[p.half[1].last];
    hipLaunchKernelGGL(p.unit_range ? k_nhwc_to_nchw_01 : k_nhwc_to_nchw, dim3((HW + 255) / 256, (unsigned)B), dim3(256), 0, st, (const float*)yo.d,
                       images_dev, p.out_ch, HW, yo.C);
    if (int rc = launch_status("k_nhwc_to_nchw")) return rc;
    s.tape = !e->frozen; s.B = (int)B;
    return WMAR_OK;
}

int wmar_vq_train_decode_backward(wmar_vq_train* e, const float* grad_images_dev, int64_t B, float* grad_zq_dev, void* stream) {
    WMAR_REQUIRE(e && grad_images_dev, "vq_train_decode_backward: null argument");
    WMAR_REQUIRE(!e->frozen, "vq_train_decode_backward: a frozen handle has no tape and no gradients (wmar_vq_train_create_frozen)");
    const VqPlan& p = e->net.plan;
    const VqHalf& h = p.half[1];
    THalf& s = e->half[1];
    WMAR_REQUIRE(s.tape, "vq_train_decode_backward: no tape (no wmar_vq_train_decode since create or the last wmar_vq_train_set_weights)");
    WMAR_REQUIRE(B == s.B, "vq_train_decode_backward: batch %lld, the tape holds %d", (long long)B, s.B);
    hipStream_t st = (hipStream_t)stream;
    s.grads = false;
    train_clear_grads(e, h);
    const int HW = p.resolution * p.resolution;
    TTensor& yo = e->t[h.last];
    if (p.unit_range) {                                         // through clamp(v, 0, 1) * 2 - 1 on the taped v
        if (int rc = run_mvq_image_backward(yo.d, grad_images_dev, yo.g, (int)B, p.out_ch, HW, yo.C, st)) return rc;
    } else {
        hipLaunchKernelGGL(k_nchw_to_nhwc, dim3((HW + 255) / 256, (unsigned)B), dim3(256), 0, st, grad_images_dev, yo.g, p.out_ch, HW, yo.C);
        if (int rc = launch_status("k_nchw_to_nhwc")) return rc;
    }
    yo.gset = true;
    if (int rc = train_backward(e, h, (int)B, grad_zq_dev != nullptr, st)) return rc;
    if (grad_zq_dev) {
        const TTensor& x0 = e->t[h.first];
        WMAR_HIP_CHECK(hipMemcpyAsync(grad_zq_dev, x0.g, x0.elems((int)B) * 4, hipMemcpyDeviceToDevice, st));
    }
    s.grads = true;
    return WMAR_OK;
}

int wmar_vq_train_get_grads(wmar_vq_train* e, const char* const* names, void* const* grads_dev, int32_t n, int32_t accumulate, void* stream) {
    WMAR_REQUIRE(e && names && grads_dev, "vq_train_get_grads: null argument");
    WMAR_REQUIRE(!e->frozen, "vq_train_get_grads: a frozen handle has no tape and no gradients (wmar_vq_train_create_frozen)");
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
