// The layer plan of a VQGAN tokenizer: the one description of each network (Taming VQGAN, RAR's MaskGIT-VQGAN) that weight loading, the
// inference engines and the taped training engine all read.  Host-only: no HIP, no allocation.
//
// A plan is two halves (0 = encoder [+ quant_conv], 1 = [post_quant_conv +] decoder), each a list of operations over numbered tensors:
// GroupNorm statistics, convolutions (with the norm they apply while loading, a residual, a stride or an upsampling), average pools and
// the middle of an AttnBlock.  References: deps/taming/modules/diffusionmodules/model.py:343-505, deps/taming/models/vqgan.py:64-73;
// deps/rar/modeling/modules/maskgit_vqgan.py, deps/rar/modeling/titok.py:41-208.
//
// Every tensor also names the buffer that holds it at inference: one of four rotating activation buffers (the block builders below say
// which, relative to the buffer of the block's input) or one of the four attention tensors.  The training engine ignores the slots and
// gives every tensor memory of its own (the tape).
#pragma once

#include <string>
#include <vector>

#include "../../include/wmar_hip.h"

namespace wmar {

enum { VQ_GN = 0, VQ_CONV = 1, VQ_ATTN = 2, VQ_POOL = 3 };
// slots 0..3 rotate; q, k, v and the attention output have buffers of their own
enum { VQ_SLOT_Q = 4, VQ_SLOT_K = 5, VQ_SLOT_V = 6, VQ_SLOT_O = 7, VQ_SLOTS = 8 };

struct VqTensor {
    int C = 0, H = 0, slot = 0;          // NHWC [B][H][H][C]; C is the stored channel count (padded to 8)
    size_t elems(int B) const { return (size_t)B * H * H * C; }
};
struct VqConvDesc { std::string name; int cin = 0, cout = 0, ks = 1, stride = 1; bool bias = true; };      // bias = false: no ".bias" tensor
struct VqNormDesc { std::string name; int C = 0; };
// GN: statistics of `in` for `norm`.  CONV: out = conv(norm ? swish?(GroupNorm(in)) : in) + res.  POOL: out = avgpool2(in).
// ATTN: out = softmax(q k^T / sqrt(C)) v; `in` is the block input (not read).
struct VqOp { int kind = 0, in = -1, out = -1, res = -1, conv = -1, norm = -1, swish = 0, up = 0, q = -1, k = -1, v = -1; };
struct VqHalf { std::vector<VqOp> ops; int first = -1, last = -1; };

struct VqPlan {
    std::string err;                     // not empty: the config was refused, nothing else is filled in
    int resolution = 0, S = 0;           // image and latent size
    int in_channels = 0, out_ch = 0;     // channels at the two image edges
    int max_batch = 0;
    bool unit_range = false;             // the network works in [0, 1]: images cross in [-1, 1] through (x + 1) / 2 and clamp(v, 0, 1) * 2 - 1
    std::vector<VqTensor> t;
    std::vector<VqConvDesc> convs;
    std::vector<VqNormDesc> norms;
    VqHalf half[2];
    // per image: the largest tensor in a rotating slot / in an attention slot / at all, the largest softmax, the zeros attention reads as a bias
    size_t rot_elems = 0, att_elems = 0, max_elems = 0, attn_nn = 0, zbias_elems = 0;
};

inline int pad8(int c) { return (c + 7) & ~7; }

// Appends operations to one half.  `rot` is the rotating slot of the current activation; slot(k) is the k-th buffer after it.
struct VqPlanBuilder {
    VqPlan& p;
    VqHalf* h = nullptr;
    int rot = 0;
    int slot(int k) const { return (rot + k) & 3; }
    int tensor(int C, int H, int s) {
        VqTensor tt; tt.C = pad8(C); tt.H = H; tt.slot = s;
        const size_t n = tt.elems(1);
        if (n > p.max_elems) p.max_elems = n;
        size_t& kind_max = s < 4 ? p.rot_elems : p.att_elems;
        if (n > kind_max) kind_max = n;
        p.t.push_back(tt);
        return (int)p.t.size() - 1;
    }
    int begin(int hidx, int C, int H) { h = &p.half[hidx]; rot = 0; return h->first = tensor(C, H, 0); }
    int gn(const std::string& name, int C, int in, int swish) {
        VqNormDesc n; n.name = name; n.C = C;
        p.norms.push_back(n);
        VqOp o; o.kind = VQ_GN; o.in = in; o.norm = (int)p.norms.size() - 1; o.swish = swish;
        h->ops.push_back(o);
        return o.norm;
    }
    // returns the output tensor, placed in slot `s`
    int conv(const std::string& name, int cin, int cout, int ks, int in, int res, int norm, int swish, int stride, int up, int s, bool bias = true) {
        VqConvDesc c; c.name = name; c.cin = cin; c.cout = cout; c.ks = ks; c.stride = stride; c.bias = bias;
        p.convs.push_back(c);
        const int Hin = p.t[in].H;
        VqOp o; o.kind = VQ_CONV; o.in = in; o.res = res; o.norm = norm; o.swish = swish; o.up = up; o.conv = (int)p.convs.size() - 1;
        o.out = tensor(cout, up ? 2 * Hin : (stride == 2 ? Hin / 2 : Hin), s);
        h->ops.push_back(o);
        return o.out;
    }
    // a conv on the trunk: into the next rotating buffer, which becomes the current one
    int step(const std::string& name, int cin, int cout, int ks, int in, int stride = 1, int up = 0, bool bias = true) {
        const int y = conv(name, cin, cout, ks, in, -1, -1, 0, stride, up, slot(1), bias);
        rot = slot(1);
        return y;
    }
    // norm_out + conv_out: two buffers on (the quant_conv behind it steps once more)
    int out_conv(const std::string& side, int cin, int cout, int ks, int X) {
        const int n = gn(side + "norm_out", cin, X, 1);
        const int y = conv(side + "conv_out", cin, cout, ks, X, -1, n, 1, 1, 0, slot(2));
        rot = slot(2);
        return y;
    }
    // Taming ResnetBlock (model.py:77-137): conv1 into slot(2), the 1 x 1 shortcut of the block INPUT into slot(3), conv2 + shortcut into slot(1)
    int res(const std::string& q, int cin, int cout, int X) {
        const int n1 = gn(q + "norm1", cin, X, 1);
        const int T = conv(q + "conv1", cin, cout, 3, X, -1, n1, 1, 1, 0, slot(2));
        const int n2 = gn(q + "norm2", cout, T, 1);
        int shortcut = X;
        if (cin != cout) shortcut = conv(q + "nin_shortcut", cin, cout, 1, X, -1, -1, 0, 1, 0, slot(3));
        const int y = conv(q + "conv2", cout, cout, 3, T, shortcut, n2, 1, 1, 0, slot(1));
        rot = slot(1);
        return y;
    }
    // MaskGIT ResnetBlock (maskgit_vqgan.py:69-87): bias-free convs; out = h + x, or h + nin_shortcut(h) with h = conv2(...) when cin != cout
    // (a 1 x 1 conv of the block OUTPUT whose input and residual are the same tensor)
    int mres(const std::string& q, int cin, int cout, int X) {
        const int n1 = gn(q + "norm1", cin, X, 1);
        const int T = conv(q + "conv1", cin, cout, 3, X, -1, n1, 1, 1, 0, slot(2), false);
        const int n2 = gn(q + "norm2", cout, T, 1);
        if (cin != cout) {
            const int A = conv(q + "conv2", cout, cout, 3, T, -1, n2, 1, 1, 0, slot(1), false);
            const int y = conv(q + "nin_shortcut", cout, cout, 1, A, A, -1, 0, 1, 0, slot(3), false);
            rot = slot(3);
            return y;
        }
        const int y = conv(q + "conv2", cout, cout, 3, T, X, n2, 1, 1, 0, slot(1), false);
        rot = slot(1);
        return y;
    }
    int pool(int X) {                                                                        // DownsamplingBlock (maskgit_vqgan.py:118-119)
        VqOp o; o.kind = VQ_POOL; o.in = X;
        o.out = tensor(p.t[X].C, p.t[X].H / 2, slot(1));
        h->ops.push_back(o);
        rot = slot(1);
        return o.out;
    }
    // AttnBlock (model.py:140-192): q, k, v and the attention output in their own buffers, proj_out + x into slot(2)
    int attn(const std::string& a, int c, int X) {
        const int H = p.t[X].H;
        const int n = gn(a + "norm", c, X, 0);
        VqOp o; o.kind = VQ_ATTN; o.in = X;
        o.q = conv(a + "q", c, c, 1, X, -1, n, 0, 1, 0, VQ_SLOT_Q);
        o.k = conv(a + "k", c, c, 1, X, -1, n, 0, 1, 0, VQ_SLOT_K);
        o.v = conv(a + "v", c, c, 1, X, -1, n, 0, 1, 0, VQ_SLOT_V);
        o.out = tensor(c, H, VQ_SLOT_O);
        h->ops.push_back(o);
        const size_t N = (size_t)H * H;
        if (N * N > p.attn_nn) p.attn_nn = N * N;
        const int y = conv(a + "proj_out", c, c, 1, o.out, X, -1, 0, 1, 0, slot(2));
        rot = slot(2);
        return y;
    }
};

inline VqPlan vq_plan_refused(const std::string& why) { VqPlan p; p.err = why; return p; }

// resolution = S << (levels - 1) with S a multiple of 8 (the convolutions work on 8 x 8 output tiles); 0 when it is not
inline int vq_latent_size(int resolution, int levels) {
    const int S = resolution >> (levels - 1);
    return (S >= 8 && S % 8 == 0 && (S << (levels - 1)) == resolution) ? S : 0;
}

// who: the create function the config came through; it prefixes the error texts that always named it
inline VqPlan plan_taming(const wmar_vq_config& c, const std::string& who) {
    if (!(c.n_levels >= 1 && c.n_levels <= 8)) return vq_plan_refused(who + ": bad ch_mult length");
    if (!(c.max_batch >= 1)) return vq_plan_refused(who + ": max_batch");
    if (c.embed_dim % 8 != 0) return vq_plan_refused("embed_dim % 8 must be 0");
    if (c.ch % 32 != 0) return vq_plan_refused("ch must be a multiple of 32 (GroupNorm has 32 groups)");
    const int L = c.n_levels, S = vq_latent_size(c.resolution, L);
    if (!S) return vq_plan_refused("latent size " + std::to_string(c.resolution >> (L - 1)) + " must be a multiple of 8");
    VqPlan p;
    p.resolution = c.resolution; p.S = S; p.in_channels = c.in_channels; p.out_ch = c.out_ch; p.max_batch = c.max_batch;
    VqPlanBuilder b{p};
    const int ch = c.ch, z = c.z_channels, E = c.embed_dim;
    auto attn_at = [&](int res) {
        for (int i = 0; i < c.n_attn_res; ++i)
            if (c.attn_resolutions[i] == res) return true;
        return false;
    };
    // ---- encoder + quant_conv (model.py:343-404)
    {
        int res = c.resolution, block_in = ch;
        int x = b.begin(0, c.in_channels, res);
        x = b.step("encoder.conv_in", c.in_channels, ch, 3, x);
        for (int lvl = 0; lvl < L; ++lvl) {
            const std::string q = "encoder.down." + std::to_string(lvl) + ".";
            block_in = ch * (lvl == 0 ? 1 : c.ch_mult[lvl - 1]);
            const int block_out = ch * c.ch_mult[lvl];
            for (int i = 0; i < c.num_res_blocks; ++i) {
                x = b.res(q + "block." + std::to_string(i) + ".", block_in, block_out, x);
                block_in = block_out;
                if (attn_at(res)) x = b.attn(q + "attn." + std::to_string(i) + ".", block_in, x);
            }
            if (lvl != L - 1) {
                x = b.step(q + "downsample.conv", block_in, block_in, 3, x, 2);
                res /= 2;
            }
        }
        x = b.res("encoder.mid.block_1.", block_in, block_in, x);
        x = b.attn("encoder.mid.attn_1.", block_in, x);
        x = b.res("encoder.mid.block_2.", block_in, block_in, x);
        x = b.out_conv("encoder.", block_in, z, 3, x);
        p.half[0].last = b.step("quant_conv", z, E, 1, x);
    }
    // ---- post_quant_conv + decoder (model.py:437-505)
    {
        int res = S, block_in = ch * c.ch_mult[L - 1];
        int x = b.begin(1, E, S);
        x = b.step("post_quant_conv", E, z, 1, x);
        x = b.step("decoder.conv_in", z, block_in, 3, x);
        x = b.res("decoder.mid.block_1.", block_in, block_in, x);
        x = b.attn("decoder.mid.attn_1.", block_in, x);
        x = b.res("decoder.mid.block_2.", block_in, block_in, x);
        for (int lvl = L - 1; lvl >= 0; --lvl) {
            const std::string q = "decoder.up." + std::to_string(lvl) + ".";
            const int block_out = ch * c.ch_mult[lvl];
            for (int i = 0; i <= c.num_res_blocks; ++i) {
                x = b.res(q + "block." + std::to_string(i) + ".", block_in, block_out, x);
                block_in = block_out;
                if (attn_at(res)) x = b.attn(q + "attn." + std::to_string(i) + ".", block_in, x);
            }
            if (lvl != 0) {
                x = b.step(q + "upsample.conv", block_in, block_in, 3, x, 1, 1);
                res *= 2;
            }
        }
        p.half[1].last = b.out_conv("decoder.", block_in, c.out_ch, 3, x);
    }
    // the zeros attention reads as a bias: max(tokens, channels) over every attention the config can name
    int amax = S, cam = 0;
    for (int i = 0; i < c.n_attn_res; ++i) amax = c.attn_resolutions[i] > amax ? c.attn_resolutions[i] : amax;
    for (int lvl = 0; lvl < L; ++lvl) cam = ch * c.ch_mult[lvl] > cam ? ch * c.ch_mult[lvl] : cam;
    p.zbias_elems = (size_t)amax * amax > (size_t)cam ? (size_t)amax * amax : (size_t)cam;
    return p;
}

inline VqPlan plan_mvq(const wmar_mvq_config& c, const std::string& who) {
    if (!(c.n_levels >= 1 && c.n_levels <= 8 && c.max_batch >= 1)) return vq_plan_refused(who + ": bad config");
    if (c.z_channels % 8 != 0 || c.hidden_channels % 32 != 0) return vq_plan_refused("z_channels % 8 and hidden_channels % 32 must be 0");
    const int R = c.n_levels, S = vq_latent_size(c.resolution, R);
    if (!S) return vq_plan_refused("latent size " + std::to_string(c.resolution >> (R - 1)) + " must be a multiple of 8");
    VqPlan p;
    p.resolution = c.resolution; p.S = S; p.in_channels = p.out_ch = c.num_channels; p.max_batch = c.max_batch; p.unit_range = true;
    VqPlanBuilder b{p};
    const int hc = c.hidden_channels, z = c.z_channels, mid = hc * c.channel_mult[R - 1];
    // ---- encoder (maskgit_vqgan.py:157-194)
    {
        int x = b.begin(0, c.num_channels, c.resolution);
        x = b.step("encoder.conv_in", c.num_channels, hc, 3, x, 1, 0, false);
        for (int lvl = 0; lvl < R; ++lvl) {
            int bi = hc * (lvl == 0 ? 1 : c.channel_mult[lvl - 1]);
            const int bo = hc * c.channel_mult[lvl];
            for (int i = 0; i < c.num_res_blocks; ++i) {
                x = b.mres("encoder.down." + std::to_string(lvl) + ".block." + std::to_string(i) + ".", bi, bo, x);
                bi = bo;
            }
            if (lvl != R - 1) x = b.pool(x);
        }
        for (int i = 0; i < c.num_res_blocks; ++i) x = b.mres("encoder.mid." + std::to_string(i) + ".", mid, mid, x);
        p.half[0].last = b.out_conv("encoder.", mid, z, 1, x);
    }
    // ---- decoder (maskgit_vqgan.py:197-245)
    {
        int x = b.begin(1, z, S);
        x = b.step("decoder.conv_in", z, mid, 3, x);
        for (int i = 0; i < c.num_res_blocks; ++i) x = b.mres("decoder.mid." + std::to_string(i) + ".", mid, mid, x);
        for (int lvl = R - 1; lvl >= 0; --lvl) {
            const std::string q = "decoder.up." + std::to_string(lvl) + ".";
            int bi = lvl == R - 1 ? mid : hc * c.channel_mult[lvl + 1];
            const int bo = hc * c.channel_mult[lvl];
            for (int i = 0; i < c.num_res_blocks; ++i) {
                x = b.mres(q + "block." + std::to_string(i) + ".", bi, bo, x);
                bi = bo;
            }
            if (lvl != 0) x = b.step(q + "upsample_conv", bo, bo, 3, x, 1, 1);
        }
        p.half[1].last = b.out_conv("decoder.", hc * c.channel_mult[0], c.num_channels, 3, x);
    }
    return p;
}

// The WAM embedder (deps/watermark_anything/modules/vae.py:176-381, models/embedder.py:45-98): Taming's encoder and decoder without
// a quantizer.  Half 0 ends at the encoder's conv_out (z_channels, no double_z); half 1 starts from the z_channels + 2 * nbits
// channels the message processor ("binary+concat") hands the decoder and ends at its conv_out (the tanh belongs to the tail kernel).
// Tensor names are the checkpoint's keys relative to `embedder.`.
inline VqPlan plan_wam(const wmar_wam_config& c, const std::string& who) {
    if (!(c.n_levels >= 1 && c.n_levels <= 8)) return vq_plan_refused(who + ": bad ch_mult length");
    if (!(c.max_batch >= 1)) return vq_plan_refused(who + ": max_batch");
    if (c.ch <= 0 || c.ch % 32 != 0) return vq_plan_refused("ch must be a multiple of 32 (GroupNorm has 32 groups)");
    if (!(c.nbits >= 1 && c.nbits <= 64)) return vq_plan_refused(who + ": nbits " + std::to_string(c.nbits) + " outside 1..64");
    if (!(c.z_channels >= 1 && c.num_res_blocks >= 1)) return vq_plan_refused(who + ": z_channels and num_res_blocks must be positive");
    if (!(c.n_attn_res >= 0 && c.n_attn_res <= 8)) return vq_plan_refused(who + ": bad attn_resolutions length");
    for (int i = 0; i < c.n_attn_res; ++i)
        if (c.attn_resolutions[i] <= 0) return vq_plan_refused(who + ": attn_resolutions must be positive");
    for (int i = 0; i < c.n_levels; ++i)
        if (c.ch_mult[i] <= 0) return vq_plan_refused(who + ": ch_mult must be positive");
    const int L = c.n_levels, S = vq_latent_size(c.resolution, L);
    if (!S) return vq_plan_refused("latent size " + std::to_string(c.resolution >> (L - 1)) + " must be a multiple of 8");
    VqPlan p;
    p.resolution = c.resolution; p.S = S; p.in_channels = 3; p.out_ch = 3; p.max_batch = c.max_batch;
    VqPlanBuilder b{p};
    const int ch = c.ch, z = c.z_channels;
    auto attn_at = [&](int res) {
        for (int i = 0; i < c.n_attn_res; ++i)
            if (c.attn_resolutions[i] == res) return true;
        return false;
    };
    {
        int res = c.resolution, block_in = ch;
        int x = b.begin(0, 3, res);
        x = b.step("encoder.conv_in", 3, ch, 3, x);
        for (int lvl = 0; lvl < L; ++lvl) {
            const std::string q = "encoder.down." + std::to_string(lvl) + ".";
            block_in = ch * (lvl == 0 ? 1 : c.ch_mult[lvl - 1]);
            const int block_out = ch * c.ch_mult[lvl];
            for (int i = 0; i < c.num_res_blocks; ++i) {
                x = b.res(q + "block." + std::to_string(i) + ".", block_in, block_out, x);
                block_in = block_out;
                if (attn_at(res)) x = b.attn(q + "attn." + std::to_string(i) + ".", block_in, x);
            }
            if (lvl != L - 1) {
                x = b.step(q + "downsample.conv", block_in, block_in, 3, x, 2);
                res /= 2;
            }
        }
        x = b.res("encoder.mid.block_1.", block_in, block_in, x);
        x = b.attn("encoder.mid.attn_1.", block_in, x);
        x = b.res("encoder.mid.block_2.", block_in, block_in, x);
        p.half[0].last = b.out_conv("encoder.", block_in, z, 3, x);
    }
    {
        const int zin = z + 2 * c.nbits;
        int res = S, block_in = ch * c.ch_mult[L - 1];
        int x = b.begin(1, zin, S);
        x = b.step("decoder.conv_in", zin, block_in, 3, x);
        x = b.res("decoder.mid.block_1.", block_in, block_in, x);
        x = b.attn("decoder.mid.attn_1.", block_in, x);
        x = b.res("decoder.mid.block_2.", block_in, block_in, x);
        for (int lvl = L - 1; lvl >= 0; --lvl) {
            const std::string q = "decoder.up." + std::to_string(lvl) + ".";
            const int block_out = ch * c.ch_mult[lvl];
            for (int i = 0; i <= c.num_res_blocks; ++i) {
                x = b.res(q + "block." + std::to_string(i) + ".", block_in, block_out, x);
                block_in = block_out;
                if (attn_at(res)) x = b.attn(q + "attn." + std::to_string(i) + ".", block_in, x);
            }
            if (lvl != 0) {
                x = b.step(q + "upsample.conv", block_in, block_in, 3, x, 1, 1);
                res *= 2;
            }
        }
        p.half[1].last = b.out_conv("decoder.", block_in, 3, 3, x);
    }
    int amax = S, cam = 0;
    for (int i = 0; i < c.n_attn_res; ++i) amax = c.attn_resolutions[i] > amax ? c.attn_resolutions[i] : amax;
    for (int lvl = 0; lvl < L; ++lvl) cam = ch * c.ch_mult[lvl] > cam ? ch * c.ch_mult[lvl] : cam;
    p.zbias_elems = (size_t)amax * amax > (size_t)cam ? (size_t)amax * amax : (size_t)cam;
    return p;
}

}  // namespace wmar
