// The host-only shape functions of the DIP conv launchers (dip_launch.h: choose_split, sm_split, the
// split-K scratch sizes, the weight-plane layout, sm_wgrad_table, sm_adj_table) over every conv node of the
// 36^2, 66^2 and 196^2 U-Nets and the 36^2 skip net, with upsample_dgrad 0 and 1: one line per call.  No GPU
// API is called; the program runs on the CPU, its host code under the sanitizers:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -I lrs-pnp-dip_amd/csrc -I include tools/conv_host_shapes.hip -o tools/conv_host_shapes
//   tools/conv_host_shapes | cmp - profiles/conv_launch/host_shapes.txt
// (the committed output is that of the functions before the launchers were reorganised)
#include <stdio.h>

#include "dip_launch.h"

static void planes(const ConvGeom &g, int Cout, bool upc, int64_t &fwd, int64_t &dgrad) {
    const WprepElems e = wprep_elems(g, Cout, upc);
    fwd = e.fwd;
    dgrad = e.dgrad;
}

static unsigned long long fnv(const std::vector<int> &v) {
    unsigned long long h = 1469598103934665603ULL;
    for (int x : v) h = (h ^ (unsigned)x) * 1099511628211ULL;
    return h;
}

static void split_line(const char *what, int M, int N, int K, int prec, bool big, int target) {
    const Split s = choose_split(M, N, K, prec, big, target);
    printf("  choose_split %s M=%d N=%d K=%d prec=%d big=%d target=%d -> S=%d kchunk=%d big=%d\n", what, M, N, K, prec,
           (int)big, target, s.S, s.kchunk, (int)s.big);
}

static void sm_line(const char *what, int M, int N, int K) {
    const Split s = sm_split(M, N, K);
    printf("  sm_split %s M=%d N=%d K=%d -> S=%d kchunk=%d part=%lld\n", what, M, N, K, s.S, s.kchunk,
           (long long)sm_part_floats(M, N, K));
}

// one conv node; returns its output size in H, W
static void conv(const char *net, int idx, int Cin, int &H, int &W, int Cout, int k, int stride, int up, int ud) {
    lrs_dip_opts o{};
    o.precision = LRS_DIP_SPLIT_BF16;
    o.upsample_dgrad = ud;
    ConvGeom g;
    const int rc = make_geom(Cin, H, W, k, stride, (k - 1) / 2, LRS_PAD_REFLECT, up, g, &o);
    printf("%s conv %d updgrad=%d Cin=%d H=%d W=%d Cout=%d k=%d stride=%d up=%d -> rc=%d Ho=%d Wo=%d ke=%d upc=%d\n", net, idx,
           ud, Cin, H, W, Cout, k, stride, up, rc, g.Ho, g.Wo, g.ke, (int)upc_conv(g));
    if (rc) return;
    const int P = g.Ho * g.Wo, kk = k * k, Kc = Cin * kk, Q = g.Hs * g.Ws;
    for (int prec : {LRS_DIP_F32, LRS_DIP_SPLIT_BF16}) {
        split_line("fwd", Cout, P, Kc, prec, false, 512);
        split_line("wgrad", Cout, Kc, P, prec, plain_unit(g), 512);
        split_line("dcol", Kc, P, Cout, prec, false, 512);
    }
    split_line("fwd_s3", Cout, P, kk * r16(Cin), LRS_DIP_SPLIT_BF16, true, kFwdSplitWg);
    split_line("wgrad_s3", Cout, Kc, P, LRS_DIP_SPLIT_BF16, true, 512);
    split_line("dgrad_s3", Cin, (g.Hu + 2 * g.pad) * (g.Wu + 2 * g.pad), kk * r16(Cout), LRS_DIP_SPLIT_BF16, true, kDgradSplitWg);
    if (g.ke) split_line("dgrad_eff", Cin, Q, g.ke * g.ke * r16(Cout), LRS_DIP_SPLIT_BF16, true, 512);
    printf("  parts gemm fwd=%lld s3 fwd=%lld conv=%lld\n", (long long)gemm_part_floats(Cout, P, Kc),
           (long long)s3_part_floats(Cout, P, kk * r16(Cin)), (long long)conv_part_floats(g, Cout));
    int64_t f, d;
    planes(g, Cout, false, f, d);
    printf("  planes upc=0 fwd=%lld dgrad=%lld\n", (long long)f, (long long)d);
    if (upc_conv(g)) {
        planes(g, Cout, true, f, d);
        printf("  planes upc=1 fwd=%lld dgrad=%lld\n", (long long)f, (long long)d);
        split_line("upc_fwd", Cout, 4 * Q, 4 * r16(Cin), LRS_DIP_SPLIT_BF16, true, kFwdSplitWg);
        split_line("upc_wgrad", Cout, 16 * Cin, Q, LRS_DIP_SPLIT_BF16, true, 512);
        printf("  parts upc=%lld\n", (long long)upc_part_floats(g, Cout));
    }
    if (!plain_unit(g) && k <= 3 && P < kImplicitMinP) {   // the small-map paths
        sm_line("fwd", Cout, P, kk * r16(Cin));
        sm_line("adjoint", Cin, Q, kk * r16(Cout));
        sm_line("wgrad", Cout, Kc, P);
        const std::vector<int> wt = sm_wgrad_table(g), at = sm_adj_table(g);
        printf("  sm_wgrad_table n=%zu fnv=%016llx\n", wt.size(), fnv(wt));
        printf("  sm_adj_table n=%zu fnv=%016llx\n", at.size(), fnv(at));
    }
    H = g.Ho;
    W = g.Wo;
}

static void unet(const char *net, int bands, int hw, int ud) {
    static const int spec[14][4] = {{128, 3, 2, 0}, {128, 3, 1, 0}, {128, 3, 2, 0}, {128, 3, 1, 0}, {128, 3, 2, 0},
                                    {128, 3, 1, 0}, {128, 3, 2, 0}, {128, 3, 1, 0}, {128, 2, 1, 1}, {128, 2, 1, 1},
                                    {128, 3, 1, 1}, {128, 3, 1, 1}, {128, 1, 1, 0}, {0, 1, 1, 0}};
    int C = bands, H = hw, W = hw;
    for (int i = 0; i < 14; ++i) {
        const int Cout = spec[i][0] ? spec[i][0] : bands;
        conv(net, i, C, H, W, Cout, spec[i][1], spec[i][2], spec[i][3], ud);
        C = Cout;
    }
}

// models/skip.py as lrspnp.dip.skip_nodes builds it: five scales of 128 channels
static void skip_level(const char *net, int &idx, int lvl, int C, int &H, int &W, int ud) {
    int hs = H, ws = W, hd = H, wd = W;
    conv(net, idx++, C, hs, ws, 128, 1, 1, 0, ud);    // skip
    conv(net, idx++, C, hd, wd, 128, 3, 2, 0, ud);    // down
    conv(net, idx++, 128, hd, wd, 128, 3, 1, 0, ud);
    if (lvl < 4) skip_level(net, idx, lvl + 1, 128, hd, wd, ud);
    H = std::min(hs, 2 * hd);   // Concat(skip, Upsample(deeper)), cropped to the smaller
    W = std::min(ws, 2 * wd);
    conv(net, idx++, 256, H, W, 128, 3, 1, 0, ud);
    conv(net, idx++, 128, H, W, 128, 1, 1, 0, ud);
}

int main() {
    for (int ud = 0; ud < 2; ++ud) {
        unet("unet36x7", 7, 36, ud);
        unet("unet66x7", 7, 66, ud);
        unet("unet196x198", 198, 196, ud);
        int idx = 0, H = 36, W = 36;
        skip_level("skip36x128", idx, 0, 128, H, W, ud);
        conv("skip36x128", idx, 128, H, W, 128, 1, 1, 0, ud);
    }
    return 0;
}
