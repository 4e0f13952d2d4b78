// Prints the layer plan (wmar_amd/csrc/vq_plan.h) of one tokenizer config as text, for tests/test_vq_plan_cpu.py.  Host-only.
//   vq_plan_dump taming ch num_res_blocks resolution in_channels out_ch z_channels embed_dim n_embed max_batch ch_mult,... [attn_res,...]
//   vq_plan_dump mvq hidden_channels num_res_blocks resolution num_channels z_channels num_embeddings max_batch channel_mult,...
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../wmar_amd/csrc/vq_plan.h"

static int ints(const char* s, int32_t* out, int cap) {
    int n = 0;
    while (s && *s && n < cap) {
        out[n++] = atoi(s);
        s = strchr(s, ',');
        if (s) ++s;
    }
    return n;
}

int main(int argc, char** argv) {
    wmar::VqPlan p;
    if (argc >= 12 && !strcmp(argv[1], "taming")) {
        wmar_vq_config c{};
        c.ch = atoi(argv[2]); c.num_res_blocks = atoi(argv[3]); c.resolution = atoi(argv[4]); c.in_channels = atoi(argv[5]);
        c.out_ch = atoi(argv[6]); c.z_channels = atoi(argv[7]); c.embed_dim = atoi(argv[8]); c.n_embed = atoi(argv[9]);
        c.max_batch = atoi(argv[10]);
        c.n_levels = ints(argv[11], c.ch_mult, 8);
        c.n_attn_res = argc > 12 ? ints(argv[12], c.attn_resolutions, 8) : 0;
        p = wmar::plan_taming(c, "vq_plan_dump");
    } else if (argc == 10 && !strcmp(argv[1], "mvq")) {
        wmar_mvq_config c{};
        c.hidden_channels = atoi(argv[2]); c.num_res_blocks = atoi(argv[3]); c.resolution = atoi(argv[4]); c.num_channels = atoi(argv[5]);
        c.z_channels = atoi(argv[6]); c.num_embeddings = atoi(argv[7]); c.max_batch = atoi(argv[8]);
        c.n_levels = ints(argv[9], c.channel_mult, 8);
        p = wmar::plan_mvq(c, "vq_plan_dump");
    } else {
        fprintf(stderr, "usage: see the head of vq_plan_dump.cpp\n");
        return 2;
    }
    if (!p.err.empty()) { printf("refused %s\n", p.err.c_str()); return 1; }
    printf("plan %d %d %d %d %d %d %zu %zu %zu %zu %zu\n", p.resolution, p.S, p.in_channels, p.out_ch, (int)p.unit_range, p.max_batch, p.rot_elems,
           p.att_elems, p.max_elems, p.attn_nn, p.zbias_elems);
    for (size_t i = 0; i < p.t.size(); ++i) printf("tensor %zu %d %d %d\n", i, p.t[i].C, p.t[i].H, p.t[i].slot);
    for (size_t i = 0; i < p.norms.size(); ++i) printf("norm %zu %s %d\n", i, p.norms[i].name.c_str(), p.norms[i].C);
    for (size_t i = 0; i < p.convs.size(); ++i) {
        const wmar::VqConvDesc& c = p.convs[i];
        printf("conv %zu %s %d %d %d %d %d\n", i, c.name.c_str(), c.cin, c.cout, c.ks, c.stride, (int)c.bias);
    }
    for (int h = 0; h < 2; ++h) {
        printf("half %d %d %d\n", h, p.half[h].first, p.half[h].last);
        for (const wmar::VqOp& o : p.half[h].ops)
            printf("op %d %d %d %d %d %d %d %d %d %d %d %d\n", h, o.kind, o.in, o.out, o.res, o.conv, o.norm, o.swish, o.up, o.q, o.k, o.v);
    }
    return 0;
}
