// DIP network engine: the net (struct lrs_dipnet), its workspace layout and its two plans.  NodePlan, per
// node: which kernels serve a conv product's forward (a CONV's, or a DECODE stage's bias-free 1x1), the
// stage tail after it, its BatchNorm and its two gradients.  StepPlan, per training step: the form of the
// loss head, what opens the step, whether sigma overlaps the first conv, which conv keeps its weight
// gradient on the main stream.  Decided once: what the shape fixes by dipnet_layout (lrs_dipnet_create),
// what the bound workspace's alignment fixes by plan_bind (lrs_dipnet_bind); the one per-call input, the
// alignment of the target and the mask, by step_head.
// dipnet_forward, weight_grad, dipnet_backward and dipnet_step (dipnet_engine.h) switch on them and
// evaluate no predicate of their own: they ask a node's kind only to tell conv products (has_conv) from BN
// and CONCAT nodes.
// Part of dipnet.hip's translation unit.
#pragma once
#include "dip_launch.h"

enum class Fwd {      // the forward product
    Direct,           // conv + BatchNorm in one k_conv_bn_dir launch (NodePlan::dg)
    Upc,              // upsampled 3 x 3 by output parity class (upc_fwd)
    Sm,               // small map: implicit GEMM on k_conv_sm, no col written
    Planes,           // implicit GEMM, or a 1x1 on k_pw, from the pre-split weight planes (conv_fwd)
    Col,              // explicit col + GEMM; a 1x1 without planes: the GEMM alone (conv_fwd)
};
enum class BnFwd {    // BatchNorm + activation after the product
    InDirect,         // inside the Fwd::Direct launch
    Reg,              // k_bn_fwd_r<nq>: register resident, finishes the product's split-K sum
    Reduce1,          // k_reduce_bn1 where the product left split-K partials, else as Generic
    Generic,          // bn_fwd (the activation alone for a conv without BatchNorm)
    ActInPw,          // a 1x1 without BatchNorm: the activation in k_pw's epilogue
    None,             // a stage tail without BatchNorm wrote the output
};
enum class Tail {     // a DECODE stage's step between the product z and its BatchNorm (plan_tail)
    None,             // a CONV; the decoder head (no upsampling, no BatchNorm, no ReLU): a bias-free CONV
    Up2Act,           // a = act(bilinear x2 of z) (up2_fwd / up2_bwd)
    Act,              // a = act(z) (dec_act_fwd_launch / dec_act_bwd_launch)
};
enum class Dgrad { None, Upc, Adjoint, Gemm };   // none (reads the input) / upc_dgrad / SmAdj gather / conv_dgrad
enum class Wgrad { Table, Im2colGemm, Upc, Gemm };   // SmWgrad gather table / k_im2col + GEMM / upc_wgrad / conv_wgrad

struct NodePlan {   // of a node with a conv product (CONV, DECODE)
    Fwd fwd = Fwd::Col;
    DirGeom dg{};
    Tail tail = Tail::None;
    bool tail_bn = false;        // a BatchNorm without activation on the tail's output a (else a is the output)
    BnFwd bn = BnFwd::Generic;   // plan_bind
    int nq = 0;                  // plan_bind: BnFwd::Reg's float4 quads per thread
    Dgrad dgrad = Dgrad::None;
    Wgrad wgrad = Wgrad::Gemm;
    bool bn_bwd_fuse = false;    // its BatchNorm backward can finish a split-K dL/dy (k_reduce_bn_bwd1)
};

enum class Head {     // the loss head of a training step
    Pw,               // last node = 1x1 conv without BN on k_pw, small map: in that conv's epilogue (PwHead); its
                      // per-workgroup sums go to hpart, reduced by k_head_reduce / k_head_loss on the side stream
    Mse,              // last node = conv without BN: loss + its activation backward in one kernel (k_mse_head)
    Generic,          // masked_mse into the last node's gradient buffer, then that node's own backward
};

struct StepPlan {     // of dipnet_step
    Head head = Head::Generic;    // dipnet_layout; Pw may become Mse for one call (step_head)
    bool begin_in_prep = false;   // plan_bind: the weight-preparation launch opens the step (else k_step_begin)
    // plan_bind: sigma overlapped with the first conv: the side stream runs the spectral-norm chain and
    // the preparation of every conv but the first, whose planes the main stream writes from the raw
    // weights (prep_head table); its BatchNorm kernel divides by the scale (plan_sn_overlap)
    bool sn_overlap = false;
    int first_conv = 0;           // plan_bind: the first node with a conv product (the node count: none)
};

// ============================================================================================
// Network engine: a DAG of conv / BN / concat nodes (the 1-Lip U-Net is a chain; the skip net
// of models/skip.py has concatenations).  Tensor 0 is the input, node i produces tensor i+1.
// ============================================================================================
struct lrs_dipnet {
    struct Node {
        lrs_dip_node d;
        int C, H, W;                  // output shape
        ConvGeom g{};                 // CONV
        CatGeom cg{};                 // CONCAT
        NodePlan plan;                // CONV, DECODE
        int64_t P = 0, Kc = 0;
        int64_t w_off = -1, b_off = -1, gm_off = -1, bt_off = -1, rs_off = -1;   // params / bn running stats (floats)
        // workspace buffers (byte offsets, -1: none)
        int64_t out_off = 0, z_off = -1, col_off = -1, mean_off = -1, istd_off = -1, wn_off = -1, grad_off = 0;
        int64_t wpre_off = -1;        // implicit convs: bf16 weight planes (wprep)
        int64_t gz_off = -1;          // conv: dL/dz (read by the side-stream weight gradient)
        // DECODE (conv 1x1 -> [bilinear x2] -> act -> [BN]) with a tail (plan.tail): z (z_off, [C][h][w], the
        // conv's map) -> a = act(up2(z)) (a_off with BN, else the output) -> BN -> output; backward ga_off =
        // dL/da (with BN, else the output gradient), gz_off = dL/dz on the conv's map.  Without a tail (the
        // head) the node is a CONV without bias and BN, loss heads included; their bias-gradient sums go to
        // gbsink_off.
        int64_t a_off = -1, ga_off = -1, gbsink_off = -1;
        int sn_index = -1;            // position in the spectral-norm table
        bool sm = false;              // small map: forward / data gradient on k_conv_sm (dip_sm.h)
        bool upc = false;             // upsampled 3 x 3: forward / data gradient by output parity class
        bool sm_dgrad = false;        // ... data gradient through the adjoint table below
        int64_t adj_off = -1;         // the lists in the workspace (shorts, sm_adj_dim)
        std::vector<int> adj;         // host copy (sm_adj_table), uploaded at bind
        int64_t wtab_off = -1;        // small map: the weight gradient's gather table (sm_wgrad_table)
        std::vector<int> wtab;
    };
    std::vector<Node> nodes;
    int C0 = 0, H = 0, W = 0;
    int64_t n_params = 0, n_bnstats = 0;
    // the workspace: byte offsets from ws, every one a multiple of 256 (dipnet_layout)
    int64_t dz_off = 0, dcol_off = 0, part_off = 0, part2_off = 0, sigma_off = 0, scale_off = 0;
    int64_t gram_off = 0, table_off = 0, misc_off = 0, bnpart_off = 0, prep_off = 0;
    int64_t part_cap = 0;     // floats of part and of part2 (the side stream's split-K partials)
    int n_prep = 0;           // convs in the per-step weight-preparation table (spectral norm and/or planes)
    StepPlan step_plan;
    int64_t prep_head_off = 0, prep_side_off = 0;   // StepPlan::sn_overlap
    // ev_sigma right after the Lanczos (the first BatchNorm needs the scale only) and ev_prep after the
    // other convs' planes (the second conv waits for it)
    hipEvent_t ev_head = nullptr, ev_sigma = nullptr, ev_prep = nullptr;
    int64_t headcnt_off = 0;         // per-channel counters of k_mse_head (zeroed at bind, reset by the kernel)
    int head_nwg = 0;                // Head::Pw
    int64_t hpart_off = 0, closs_off = 0;
    size_t ws_bytes = 0;
    int n_sn = 0;
    int64_t max_w = 0;
    bool implicit = false;   // convs gather im2col inside the split-bf16 GEMM (no col buffers)
    float *params = nullptr, *grads = nullptr, *am = nullptr, *av = nullptr, *bnstats = nullptr;
    char *ws = nullptr;
    hipGraphExec_t gexec = nullptr;
    hipGraph_t graph = nullptr;
    // weight gradients run on a side stream beside the data-gradient chain (fork per conv node
    // after its BN backward, join before Adam) at every size: beside the concurrent sparse-coding kernel
    // the second stream keeps the DIP its share of the chip (configs[2] 4.73 -> 5.19 outer it/s,
    // round 1); at 36^2 it was slower in round 1 (1.03 -> 1.19 ms per step) and is faster since the
    // small-map fork points pair up (round 4, interleaved: 0.729 -> 0.676 ms per step)
    hipStream_t side = nullptr;   // the one for the current call's priority (one of sides)
    std::vector<std::pair<int, hipStream_t>> sides;   // (priority, stream): one per priority seen
    std::vector<hipEvent_t> ev_fork;
    hipEvent_t ev_join = nullptr;
    struct Key {   // (no padding: compared with memcmp)
        const void *x, *t, *m, *es, *ring;
        int64_t mstride;   // the mask mode: [P] and [C][P] at one pointer are different graphs
        float lr, b1, b2, eps;
        int32_t fr_top, fr_left, fr_H, fr_W;   // the frame (lrs_dipnet_set_frame): another loss mean and ring
    } key{};
    bool have_key = false;
    // The image inside the output (lrs_dipnet_set_frame; the whole output until it is called:
    // lrs_dipnet_create).  framed: the loss heads average over the interior's n_mean() elements and the
    // early-stopping ring holds the interior only; not framed: the step is what it was without a frame.
    int fr_top = 0, fr_left = 0, fr_H = 0, fr_W = 0;
    bool framed = false;
    int64_t n_mean() const {
        const Node &L = nodes.back();
        return framed ? (int64_t)L.C * fr_H * fr_W : (int64_t)L.C * L.P;
    }
    lrs_dip_opts opts{};      // fixed at creation (precision, upsampled data-gradient form)
    float ln_lambda = 1.0f;   // W_used = W / max(1, sigma / ln_lambda)   (lipschitz_constraint_layer.py:42-44)

    // typed views of the bound workspace (callers check ws first)
    template <class T> T *at(int64_t off) const { return (T *)(ws + off); }
    float *f(int64_t off) const { return at<float>(off); }
    double *gram() const { return at<double>(gram_off); }
    SnConv *table() const { return at<SnConv>(table_off); }
    ConvPrep *prep() const { return at<ConvPrep>(prep_off); }
    ConvPrep *prep_head() const { return at<ConvPrep>(prep_head_off); }
    ConvPrep *prep_side() const { return at<ConvPrep>(prep_side_off); }
    int *headcnt() const { return at<int>(headcnt_off); }
    double *loss_acc() const { return at<double>(misc_off); }
    int *step() const { return at<int>(misc_off + 8); }
    double *bnpart() const { return at<double>(bnpart_off); }
    double *hpart() const { return at<double>(hpart_off); }
    double *closs() const { return at<double>(closs_off); }
    // a node's bias in params, or its gradient in grads (base); NULL where it has none (DECODE, BN)
    float *bias_in(float *base, const Node &N) const { return N.b_off >= 0 ? base + N.b_off : nullptr; }
    // where a loss head puts the last node's bias gradient (a DECODE head has no bias: a scratch row)
    float *head_gbias(const Node &N) const { return N.b_off >= 0 ? grads + N.b_off : f(N.gbsink_off); }
    const float *tensor(int t, const float *x) const { return t == 0 ? x : f(nodes[t - 1].out_off); }
    int tC(int t) const { return t == 0 ? C0 : nodes[t - 1].C; }
    int tH(int t) const { return t == 0 ? H : nodes[t - 1].H; }
    int tW(int t) const { return t == 0 ? W : nodes[t - 1].W; }

    // ---- launch arguments of a conv node ----------------------------------------------------
    // the one-workgroup-per-channel BatchNorm forward kernels (vec: their float4 form)
    BnArgs bn_args(const Node &N, int vec) const {
        return {f(N.z_off), f(N.out_off), params + N.gm_off, params + N.bt_off, f(N.mean_off), f(N.istd_off),
                bnstats + N.rs_off, bnstats + N.rs_off + N.C, nullptr, N.C, (int)N.P, 1, (int)N.P, 1, N.d.act, kBnEps,
                kBnMomentum, N.d.bn == 2 ? 1 : 0, vec};
    }
    // k_reduce_bn_bwd1: dL/dy arrives as split-K partials
    BnBwdArgs bn_bwd_args(const Node &N) const {
        return {nullptr, f(N.out_off), f(N.z_off), params + N.gm_off, f(N.mean_off), f(N.istd_off), f(N.gz_off),
                grads + N.gm_off, grads + N.bt_off, bias_in(grads, N), nullptr, N.C, (int)N.P, 1, (int)N.P, 1, N.d.act,
                N.d.bn == 2 ? 1 : 0, 0, 0, params + N.bt_off};
    }
    // ---- the generic BatchNorm (+ activation) of any node: bn_fwd / bn_bwd on tensors as stored ----
    // in -> the node's output (without BatchNorm parameters the activation alone)
    int node_bn_fwd(const Node &N, const float *in, int act, hipStream_t st) const {
        const bool bn = N.gm_off >= 0;
        return bn_fwd(in, f(N.out_off), bn ? params + N.gm_off : nullptr, bn ? params + N.bt_off : nullptr,
                      f(N.mean_off), f(N.istd_off), bn ? bnstats + N.rs_off : nullptr,
                      bn ? bnstats + N.rs_off + N.C : nullptr, N.C, N.P, act, kBnEps, kBnMomentum, bnpart(), st,
                      N.d.bn == 2 ? 1 : 0);
    }
    // the node's output gradient -> dst (+)= dL/d(in), and the gradients of gamma, beta and the bias it has
    int node_bn_bwd(const Node &N, const float *in, int act, float *dst, int accum, hipStream_t st) const {
        const bool bn = N.gm_off >= 0;
        return bn_bwd(f(N.grad_off), f(N.out_off), in, bn ? params + N.gm_off : nullptr, f(N.mean_off), f(N.istd_off),
                      dst, bn ? grads + N.gm_off : nullptr, bn ? grads + N.bt_off : nullptr, bias_in(grads, N), N.C, N.P,
                      act, bnpart(), st, N.d.bn == 2 ? 1 : 0, accum, bn ? params + N.bt_off : nullptr);
    }
    // the weights the products read (W / scale under spectral norm) and the scale a weight gradient
    // divides by (NULL without spectral norm)
    struct ConvW { const float *w, *div; };
    ConvW conv_w(const Node &N) const {
        const bool sn = N.sn_index >= 0;
        return {sn ? f(N.wn_off) : params + N.w_off, sn ? f(scale_off) + N.sn_index : nullptr};
    }
};

namespace {

// the largest map (output pixels) whose last 1x1 conv takes the loss head into its epilogue (PwHead): only
// on small maps, 36^2 step 0.578 -> 0.571 ms, but 196^2 1.187 -> 1.192 ms (3 interleaved rounds,
// profiles/r06/ab/fused_head.txt): there the epilogue's extra 60 MB (target in, gz out) lengthens the
// 481-workgroup conv by more than the separate k_mse_head launch costs
constexpr int64_t kHeadPwMaxP = 4096;

// the largest small map (output pixels) whose conv + BatchNorm run as one k_conv_bn_dir launch:
// the 9^2 and smaller maps (36^2 step 0.635 -> 0.621 ms; 196^2 within noise; with the 13^2 / 18^2
// maps too both are slower: 196^2 +28 us, 36^2 +3 us; 2 interleaved rounds, profiles/r05/dir/)
constexpr int64_t kDirMaxP = 100;
// (so the overlapped sigma's first conv, >= kForkBigP pixels, is never the direct launch, and its
// BatchNorm never the one-workgroup form: only BnFwd::Reg finishes its split-K sum)
static_assert(kDirMaxP < kForkBigP && 4 * kBn1Threads < kForkBigP, "the overlapped first conv's forms");

// ---- the plan: the only place that names these predicates -------------------------------------
using Node = lrs_dipnet::Node;

// a node with a conv product: weights, planes, weight and data gradients
inline bool has_conv(const Node &N) { return N.d.kind == LRS_NODE_CONV || N.d.kind == LRS_NODE_DECODE; }

// what follows the product: a DECODE stage that upsamples, normalises or rectifies runs the decoder's own
// kernels on z; any other (the head) is a bias-free CONV, loss heads included
void plan_tail(Node &N) {
    const bool tail = N.d.kind == LRS_NODE_DECODE && (N.d.upsample || N.d.bn || N.d.act == LRS_ACT_RELU);
    N.plan.tail = !tail ? Tail::None : N.d.upsample ? Tail::Up2Act : Tail::Act;
    N.plan.tail_bn = tail && N.d.bn;
}

void plan_fwd(Node &N) {
    const bool on_planes = plain_unit(N.g) ? N.wpre_off >= 0 : N.col_off < 0;
    if (N.d.bn && N.sm && N.P <= kDirMaxP && dir_geom(N.g, N.plan.dg)) N.plan.fwd = Fwd::Direct;
    else if (N.upc) N.plan.fwd = Fwd::Upc;
    else if (N.sm) N.plan.fwd = Fwd::Sm;
    else N.plan.fwd = on_planes ? Fwd::Planes : Fwd::Col;
}

// aligned: the workspace is 16-byte aligned, and with it (every offset a multiple of 256) z, the
// output and the split-K partials the float4 kernels read
void plan_bn_fwd(Node &N, bool aligned) {
    NodePlan &p = N.plan;
    const bool bn = N.d.bn != 0;
    p.nq = 0;
    // after a tail the BatchNorm reads a as stored: nothing of the product is left to finish
    if (p.tail != Tail::None) p.bn = p.tail_bn ? BnFwd::Generic : BnFwd::None;
    else if (p.fwd == Fwd::Direct) p.bn = BnFwd::InDirect;
    else if (!bn && p.fwd == Fwd::Planes && plain_unit(N.g)) p.bn = BnFwd::ActInPw;
    else if (bn && (p.nq = bn_reg_q(N.P, aligned && N.P % 4 == 0)) > 0) p.bn = BnFwd::Reg;
    else p.bn = (bn && bn_one_wg(N.P)) ? BnFwd::Reduce1 : BnFwd::Generic;
}

void plan_grads(Node &N) {
    N.plan.dgrad = N.d.in0 == 0 ? Dgrad::None : N.upc ? Dgrad::Upc : N.sm_dgrad ? Dgrad::Adjoint : Dgrad::Gemm;
    N.plan.wgrad = N.sm ? (N.wtab_off >= 0 ? Wgrad::Table : Wgrad::Im2colGemm) : N.upc ? Wgrad::Upc : Wgrad::Gemm;
    // (a tail's BatchNorm backward takes dL/dy as stored)
    N.plan.bn_bwd_fuse = N.plan.tail == Tail::None && N.d.bn && bn_one_wg(N.P);
}

// Sigma beside the first conv: a spectrally normalised first conv on the network input, read from
// weight planes, whose BatchNorm kernel finishes its split-K sum of at least 2 partials and divides
// by the scale.  Only where that conv is long enough to hide the side chain (~70 us at 196^2: the
// Gram reduce, Lanczos and the other convs' planes); at 36^2 the 18^2 first conv takes 7 us and the
// overlap measured slower (0.647 -> 0.663 ms per step).
bool plan_sn_overlap(const lrs_dipnet *net) {
    const Node &N0 = net->nodes[0];
    const bool implicit = N0.plan.fwd == Fwd::Sm || (N0.plan.fwd == Fwd::Planes && !plain_unit(N0.g));
    if (N0.d.kind != LRS_NODE_CONV || N0.d.in0 != 0 || N0.sn_index < 0 || !implicit || N0.plan.bn != BnFwd::Reg)
        return false;
    const int K = N0.g.k * N0.g.k * r16(N0.g.Cin);
    const int S = N0.plan.fwd == Fwd::Sm ? sm_split(N0.C, (int)N0.P, K).S
                                        : choose_split(N0.C, (int)N0.P, K, LRS_DIP_SPLIT_BF16, true, kFwdSplitWg).S;
    return S >= 2 && N0.P >= kForkBigP;
}

// the alignment-dependent part, once the workspace is known, and the step's
void plan_bind(lrs_dipnet *net) {
    StepPlan &sp = net->step_plan;
    for (Node &N : net->nodes)
        if (has_conv(N)) plan_bn_fwd(N, al16(net->ws));
    sp.sn_overlap = plan_sn_overlap(net);
    sp.begin_in_prep = net->n_prep > 0;
    sp.first_conv = 0;
    while (sp.first_conv < (int)net->nodes.size() && !has_conv(net->nodes[sp.first_conv])) ++sp.first_conv;
}

// float4 mask loads: row c starts at mask + c * mstride, 16-B aligned for every c when the base is
// and the stride is a multiple of 4 floats (0, or P with P % 4 == 0)
bool mask_al16(const float *mask, int64_t mstride) { return !mask || (al16(mask) && mstride % 4 == 0); }

// The loss head of one call: k_pw's epilogue takes its float4 form when P % 4 == 0 and reads the target
// and the mask rows as float4 there; a [C][P] mask with P % 4 != 0 has unaligned rows and takes
// k_mse_head's scalar path instead, as does any unaligned target or mask.
Head step_head(const lrs_dipnet *net, const float *target, const float *mask, int64_t mstride) {
    const Head h = net->step_plan.head;
    return (h == Head::Pw && !(mask_al16(mask, mstride) && al16(target))) ? Head::Mse : h;
}

// ---- the workspace layout -------------------------------------------------------------------
struct Bump {   // byte offsets in allocation order; each extent is rounded up to its alignment
    int64_t p;
    explicit Bump(int64_t at) : p(at) {}
    int64_t take(int64_t bytes, int64_t align = 256) { const int64_t at = p; p += round_up(bytes, align); return at; }
    int64_t floats(int64_t n) { return take(n * (int64_t)sizeof(float)); }
    int64_t planes(int64_t bf16_elems) { return floats((bf16_elems + 1) / 2); }
};

// Node shapes, parameter offsets, workspace offsets and the shape-dependent plan of a new net.
int dipnet_layout(lrs_dipnet *net, const lrs_dip_node *nodes, int n_nodes) {
    const lrs_dip_opts &o = net->opts;
    Bump ws(0);
    int64_t pofs = 0, rofs = 0, max_dz = 0, max_dcol = 0, part = 0, max_bnpart = 0;
    for (int i = 0; i < n_nodes; ++i) {
        Node N;
        N.d = nodes[i];
        const int t0 = N.d.in0;
        if (t0 < 0 || t0 > i) return LRS_E_INVALID;
        if (N.d.act != LRS_ACT_NONE && N.d.act != LRS_ACT_LRELU && N.d.act != LRS_ACT_SIGMOID &&
            !(N.d.act == LRS_ACT_RELU && N.d.kind == LRS_NODE_DECODE))
            return LRS_E_INVALID;
        // bilinear upsampling is the DECODE stage's alone (every other kind: non-zero = nearest)
        if (N.d.upsample == LRS_UP_BILINEAR && (N.d.kind == LRS_NODE_CONV || N.d.kind == LRS_NODE_CONCAT))
            return LRS_E_INVALID;
        if (N.d.bn < 0 || N.d.bn > 2) return LRS_E_INVALID;
        const int ci = net->tC(t0), hi = net->tH(t0), wi = net->tW(t0);
        if (has_conv(N)) {
            // a DECODE stage's product is a bias-free 1x1 on the input's map; its tail may double the map
            const bool dec = N.d.kind == LRS_NODE_DECODE;
            const int up = dec && N.d.upsample ? 2 : 1;
            if (N.d.cout <= 0) return LRS_E_INVALID;
            if (dec) {
                if (N.d.k != 1 || N.d.stride != 1 || N.d.pad != 0 || N.d.sn != 0 || N.d.bn == LRS_BN_LIP ||
                    (N.d.upsample != 0 && N.d.upsample != LRS_UP_BILINEAR))
                    return LRS_E_UNSUPPORTED;
                if (N.d.act == LRS_ACT_SIGMOID && (N.d.upsample || N.d.bn)) return LRS_E_INVALID;   // the head only
            }
            if (const int rc = make_geom(ci, hi, wi, N.d.k, N.d.stride, N.d.pad, dec ? LRS_PAD_ZERO : N.d.pad_mode,
                                         dec ? 0 : N.d.upsample, N.g, &o))
                return rc;
            if (dec && ((int64_t)up * hi > INT32_MAX / 4 / ((int64_t)up * wi) || N.d.cout > 65535))
                return LRS_E_UNSUPPORTED;
            N.C = N.d.cout; N.H = up * N.g.Ho; N.W = up * N.g.Wo;
            N.P = (int64_t)N.H * N.W;
            const int64_t Pz = (int64_t)N.g.Ho * N.g.Wo;   // the product's map (N.P but under a doubling tail)
            N.Kc = (int64_t)ci * N.d.k * N.d.k;
            N.w_off = pofs; pofs += N.C * N.Kc;
            if (!dec) { N.b_off = pofs; pofs += N.C; }
            plan_tail(N);
            const bool tail = N.plan.tail != Tail::None;
            if (N.d.sn) {
                if ((N.Kc < N.C ? N.Kc : N.C) > kSnMaxDim) return LRS_E_UNSUPPORTED;
                N.sn_index = net->n_sn++;
                N.wn_off = ws.floats(N.C * N.Kc);
                if (N.C * N.Kc > net->max_w) net->max_w = N.C * N.Kc;
            }
            const int64_t planes = wprep_elems(N.g, N.C, false).total();
            const bool planes_fit = planes < INT32_MAX / 3;   // k_conv_prep's 32-bit plane indices
            if (plain_unit(N.g)) {
                if (net->implicit && pw_ok(N.g, N.C) && Pz >= kImplicitMinP && planes_fit)
                    N.wpre_off = ws.planes(planes);   // 1x1 on k_pw: its pre-split weight planes
            } else if (!(net->implicit && conv_implicit_ok(N.g, N.C) && N.P >= kImplicitMinP)) {
                // col: the weight gradient's explicit im2col (written in the backward for a
                // small-map conv, whose forward gathers it inside k_conv_sm)
                N.col_off = ws.floats(N.Kc * N.P);
                if (net->implicit && N.d.k <= 3 && conv_implicit_ok(N.g, N.C) && planes_fit) {
                    N.sm = true;
                    N.wpre_off = ws.planes(planes);
                    if (N.P <= kSmWgradOneLaunchP) {
                        N.wtab = sm_wgrad_table(N.g);
                        N.wtab_off = ws.floats((int64_t)N.wtab.size());
                    }
                    if (t0 > 0) {
                        N.adj = sm_adj_table(N.g);
                        N.sm_dgrad = !N.adj.empty();
                        if (N.sm_dgrad) N.adj_off = ws.floats((int64_t)N.adj.size());
                    }
                }
            } else {
                N.upc = upc_conv(N.g);
                const int64_t elems = wprep_elems(N.g, N.C, N.upc).total();
                if (elems >= INT32_MAX / 3) return LRS_E_UNSUPPORTED;
                N.wpre_off = ws.planes(elems);
            }
            if (!plain_unit(N.g)) max_dcol = std::max(max_dcol, N.Kc * N.P);
            if (N.d.bn || tail) N.z_off = ws.floats(N.C * Pz);
            if (N.plan.tail_bn) {
                N.a_off = ws.floats(N.C * N.P);
                N.ga_off = ws.floats(N.C * N.P);
            }
            if (dec && !tail) N.gbsink_off = ws.floats(N.C);
            N.gz_off = ws.floats(N.C * Pz);
            part = std::max({part, conv_part_floats(N.g, N.C), N.upc ? upc_part_floats(N.g, N.C) : 0});
            // (dz serves a BN node on the input alone; a CONV's share stays so that no offset moves)
            if (!dec) max_dz = std::max(max_dz, N.C * N.P);
            plan_fwd(N);
            plan_grads(N);
        } else if (N.d.kind == LRS_NODE_BN) {
            if (!N.d.bn) N.d.bn = 1;
            N.C = ci; N.H = hi; N.W = wi;
            N.P = (int64_t)hi * wi;
            max_dz = std::max(max_dz, N.C * N.P);
        } else if (N.d.kind == LRS_NODE_CONCAT) {
            const int t1 = N.d.in1;
            if (t1 < 0 || t1 > i) return LRS_E_INVALID;
            auto &cg = N.cg;
            cg.Ca = ci; cg.Ha = hi; cg.Wa = wi;
            cg.Cb = net->tC(t1); cg.Hb = net->tH(t1); cg.Wb = net->tW(t1); cg.upb = N.d.upsample ? 1 : 0;
            const int hb = cg.upb ? 2 * cg.Hb : cg.Hb, wb = cg.upb ? 2 * cg.Wb : cg.Wb;
            cg.H = hi < hb ? hi : hb; cg.W = wi < wb ? wi : wb;
            cg.oay = (hi - cg.H) / 2; cg.oax = (wi - cg.W) / 2;
            cg.oby = (hb - cg.H) / 2; cg.obx = (wb - cg.W) / 2;
            N.C = cg.Ca + cg.Cb; N.H = cg.H; N.W = cg.W;
            N.P = (int64_t)N.H * N.W;
            N.d.bn = 0;
        } else {
            return LRS_E_INVALID;
        }
        // BN partials: every BN and every conv (its bias gradient is reduced the same way)
        if (N.d.bn || has_conv(N)) max_bnpart = std::max(max_bnpart, bn_part_doubles(N.C, N.P));
        if (N.d.bn) {
            N.gm_off = pofs; pofs += N.C;
            N.bt_off = pofs; pofs += N.C;
            N.rs_off = rofs; rofs += 2 * N.C;
        }
        if (N.d.bn || has_conv(N)) {   // without BN: unused placeholders (the kernels take them)
            N.mean_off = ws.floats(N.C);
            N.istd_off = ws.floats(N.C);
        }
        N.out_off = ws.floats((int64_t)N.C * N.P);
        N.grad_off = ws.floats((int64_t)N.C * N.P);
        net->nodes.push_back(N);
    }
    const Node &Lh = net->nodes.back();
    const int n_sn = net->n_sn;
    net->n_params = pofs;
    net->n_bnstats = rofs;
    net->dz_off = ws.floats(max_dz);
    net->dcol_off = ws.floats(max_dcol);
    net->part_off = ws.floats(part);
    net->part2_off = ws.floats(part);
    net->part_cap = part;
    net->sigma_off = ws.floats(std::max(n_sn, 1));
    net->scale_off = ws.floats(std::max(n_sn, 1));
    net->gram_off = ws.take((int64_t)n_sn * kSnGramDoubles * (int64_t)sizeof(double), 8);
    net->bnpart_off = ws.take(std::max<int64_t>(max_bnpart, 1) * (int64_t)sizeof(double));
    net->table_off = ws.take(std::max(n_sn, 1) * (int64_t)sizeof(SnConv));
    for (const Node &N : net->nodes)
        if (has_conv(N) && (N.sn_index >= 0 || N.wpre_off >= 0)) ++net->n_prep;
    const int64_t prep_bytes = std::max(net->n_prep, 1) * (int64_t)sizeof(ConvPrep);
    net->prep_off = ws.take(prep_bytes);
    net->prep_head_off = ws.take(256);   // one ConvPrep
    net->prep_side_off = ws.take(prep_bytes);
    const bool head_mse = has_conv(Lh) && Lh.plan.tail == Tail::None && Lh.d.bn == 0 && Lh.C <= 65535;
    const bool head_pw = head_mse && plain_unit(Lh.g) && Lh.wpre_off >= 0 && Lh.P <= kHeadPwMaxP;
    net->step_plan.head = head_pw ? Head::Pw : head_mse ? Head::Mse : Head::Generic;
    if (head_pw) {
        net->hpart_off = ws.take(2 * (int64_t)Lh.C * ((Lh.P + 63) / 64) * 8);   // [2][C][<= ceil(P / 64) workgroups]
        net->closs_off = ws.take((int64_t)Lh.C * 8);
    }
    net->headcnt_off = ws.take((int64_t)(Lh.C + 1) * 4);   // C per-channel counters + the channel counter
    net->misc_off = ws.take(256);
    net->ws_bytes = (size_t)ws.p;
    net->ev_fork.assign(net->nodes.size(), nullptr);   // side stream + events: ensure_side()
    return LRS_OK;
}

}  // namespace
