// DIP network engine: one training step of a bound net (struct lrs_dipnet, dipnet_plan.h) as launches on
// two streams: the forward, the loss head, the backward with the weight gradients on a side stream, Adam.
// Every per-node choice is read from NodePlan and every per-step choice from StepPlan (dipnet_plan.h);
// the functions here switch on them and evaluate no predicate of their own.  A stand-alone forward or
// backward (lrs_dipnet_forward / lrs_dipnet_backward) is the same walk with a default FwdStep / BwdStep.
// Part of dipnet.hip's translation unit.
#pragma once
#include "dipnet_plan.h"

namespace {

// The mask's channel count (1: [P], broadcast over the channels; C: per element [C][P]) -> its row
// stride in floats (0 / P; 0 without a mask); -1 for any other count.
int64_t mask_stride(const float *mask, int mask_channels, int C, int64_t P) {
    if (mask_channels != 1 && mask_channels != C) return -1;
    return (mask && mask_channels == C && C > 1) ? P : 0;
}

// Head::Generic, and the masked-MSE entry points.
// n_mean: the element count of the mean (C P, or fewer for a framed output: k_masked_mse_n)
int masked_mse(const float *out, const float *target, const float *mask, int mask_channels, int C, int64_t P,
               int64_t n_mean, float *gout, double *loss_acc, void *stream) {
    if (!out || !target || !loss_acc || C <= 0 || P <= 0 || n_mean <= 0 || n_mean > (int64_t)C * P) return LRS_E_INVALID;
    const int64_t mstride = mask_stride(mask, mask_channels, C, P);
    if (mstride < 0) return LRS_E_INVALID;
    const int vec = (P % 4 == 0 && al16(out) && al16(target) && mask_al16(mask, mstride) && (!gout || al16(gout))) ? 1 : 0;
    int64_t S = (512 + C - 1) / C;   // ~512 workgroups over the C channels (fewer loss atomics)
    S = std::max<int64_t>(1, std::min<int64_t>(S, (P + 1023) / 1024));
    int64_t chunk = (P + S - 1) / S;
    if (vec) chunk = (chunk + 3) & ~(int64_t)3;
    if (chunk > INT32_MAX || C > 65535) return LRS_E_UNSUPPORTED;
    if (n_mean == (int64_t)C * P)
        hipLaunchKernelGGL(k_masked_mse, dim3((unsigned)S, (unsigned)C), dim3(256), 0, (hipStream_t)stream, out, target,
                           mask, mstride, C, P, (int)chunk, vec, gout, loss_acc);
    else
        hipLaunchKernelGGL(k_masked_mse_n, dim3((unsigned)S, (unsigned)C), dim3(256), 0, (hipStream_t)stream, out, target,
                           mask, mstride, n_mean, P, (int)chunk, vec, gout, loss_acc);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// Head::Mse: k_mse_head over the last node (conv without BN): gz and the bias gradient of that node, + loss
int mse_head(lrs_dipnet *net, const float *out, const float *target, const float *mask, int64_t mstride,
             hipStream_t st) {
    const auto &N = net->nodes.back();
    float *gz = net->f(N.gz_off);
    const int64_t P = N.P;
    const int vec = (P % 4 == 0 && al16(out) && al16(target) && mask_al16(mask, mstride) && al16(gz)) ? 1 : 0;
    int64_t S = bn_split(P);   // ~4096 pixels per workgroup
    int64_t chunk = (P + S - 1) / S;
    if (vec) chunk = (chunk + 3) & ~(int64_t)3;
    S = (P + chunk - 1) / chunk;
    // partials: bias [C][S], loss [C][S], channel losses [C]  (bn_part_doubles = 3 C bn_split(P))
    if (chunk > INT32_MAX || P > INT32_MAX || 2 * (int64_t)N.C * S + N.C > bn_part_doubles(N.C, P))
        return LRS_E_UNSUPPORTED;
    if (!net->framed)
        hipLaunchKernelGGL(k_mse_head, dim3((unsigned)S, (unsigned)N.C), dim3(256), 0, st, out, target, mask, mstride, N.C,
                           P, (int)chunk, vec, N.d.act, gz, net->loss_acc(), net->bnpart(), net->headcnt(),
                           net->head_gbias(N));
    else
        hipLaunchKernelGGL(k_mse_head_n, dim3((unsigned)S, (unsigned)N.C), dim3(256), 0, st, out, target, mask, mstride,
                           N.C, P, (int)chunk, vec, N.d.act, gz, net->loss_acc(), net->bnpart(), net->headcnt(),
                           net->head_gbias(N), net->n_mean());
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// ---- forward ----------------------------------------------------------------------------------
// workgroups per conv of the per-step weight preparation
constexpr int kPrepWg = 512;

// What a training step adds to the forward; the defaults are a stand-alone forward.
struct FwdStep {
    bool begin = false;       // the weight-preparation launch opens the step (StepPlan::begin_in_prep)
    // the overlapped sigma (StepPlan::sn_overlap, sn_overlap_head): the spectral-norm chain and the weight
    // preparation were enqueued by the caller (the first conv's planes from the raw weights on st, the rest
    // on the side stream, which records ev_sigma); the first conv runs on the raw planes and st waits for
    // ev_sigma before its BatchNorm kernel, which divides by the scale.
    bool raw_first = false;
    const PwHead *head = nullptr;   // Head::Pw: the loss head in the last conv's epilogue
};

int conv_fwd_node(lrs_dipnet *net, size_t i, const float *x, hipStream_t st, const FwdStep &fs) {
    auto &N = net->nodes[i];
    const NodePlan &pl = N.plan;
    float *out = net->f(N.out_off);
    // z: the product (the output itself where neither a BatchNorm nor a stage tail reads it)
    float *z = N.z_off >= 0 ? net->f(N.z_off) : out, *part = net->f(net->part_off);
    const float *xin = net->tensor(N.d.in0, x), *w = net->conv_w(N).w, *bias = net->bias_in(net->params, N);
    const __bf16 *wp = N.wpre_off >= 0 ? net->at<__bf16>(N.wpre_off) : nullptr;
    // these BatchNorm kernels finish the product's split-K sum themselves
    int nsplit = 1;
    int *ns = (pl.bn == BnFwd::Reg || pl.bn == BnFwd::Reduce1) ? &nsplit : nullptr;
    int rc = LRS_OK;
    switch (pl.fwd) {
    case Fwd::Direct: dir_launch(N.g, pl.dg, xin, w, bias, net->bn_args(N, 0), st); break;
    case Fwd::Upc: rc = upc_fwd(N.g, xin, wp, bias, N.C, z, part, net->part_cap, st, ns); break;
    case Fwd::Sm: {
        const int kk = N.g.k * N.g.k, Cp = r16(N.g.Cin);
        rc = sm_launch(SmPre{wp, (int64_t)N.C * kk * Cp, kk * Cp, N.C},
                       SmFwd{xin, N.g.Cin * N.g.Hs * N.g.Ws * 4, N.g, Cp, nullptr}, z, bias, N.C, (int)N.P, kk * Cp, 0,
                       part, net->part_cap, st, ns);
        break;
    }
    case Fwd::Planes:
    case Fwd::Col: {
        const bool act_pw = pl.bn == BnFwd::ActInPw;
        rc = conv_fwd(N.g, xin, w, bias, N.C, N.col_off >= 0 ? net->f(N.col_off) : nullptr, z, part, net->part_cap, st,
                      wp, ns, act_pw ? N.d.act : 0, (act_pw && i + 1 == net->nodes.size()) ? fs.head : nullptr);
        break;
    }
    }
    if (rc) return rc;
    // the DECODE stage's tail: a = act([bilinear x2] z); its BatchNorm, if any, has no activation left
    const float *bn_in = z;
    int bn_act = N.d.act;
    if (pl.tail != Tail::None) {
        float *a = pl.tail_bn ? net->f(N.a_off) : out;
        rc = pl.tail == Tail::Up2Act ? up2_fwd(z, N.C, N.g.Ho, N.g.Wo, N.d.act, a, st)
                                     : dec_act_fwd_launch(z, a, (int64_t)N.C * N.P, N.d.act, st);
        if (rc) return rc;
        bn_in = a;
        bn_act = LRS_ACT_NONE;
    }
    // the raw-weight first conv (its product left >= 2 partials: plan_sn_overlap): its BatchNorm
    // kernel divides by the scale
    const float *sdiv = nullptr;
    if (fs.raw_first && i == 0) {
        const hipError_t e = hipStreamWaitEvent(st, net->ev_sigma, 0);
        if (e != hipSuccess) return (int)e;
        sdiv = net->f(net->scale_off) + N.sn_index;
    }
    const float *pp = nsplit > 1 ? (const float *)part : nullptr;
    if (pl.bn == BnFwd::Reg) {
        launch_bn_fwd_r(pl.nq, pp, nsplit, bias, net->bn_args(N, 1), sdiv, st);
    } else if (pl.bn == BnFwd::Reduce1 && nsplit > 1) {
        launch_reduce_bn1(pp, nsplit, bias, net->bn_args(N, 0), sdiv, st);
    } else if (pl.bn == BnFwd::Reduce1 || pl.bn == BnFwd::Generic) {
        rc = net->node_bn_fwd(N, bn_in, bn_act, st);
    }
    return rc;
}

int bn_fwd_node(lrs_dipnet *net, const Node &N, const float *x, hipStream_t st) {
    return net->node_bn_fwd(N, net->tensor(N.d.in0, x), N.d.act, st);
}

int concat_fwd_node(lrs_dipnet *net, const Node &N, const float *x, hipStream_t st) {
    float *out = net->f(N.out_off);
    const int q = N.cg.H * ((N.cg.W + 3) / 4);
    if (N.cg.Ca + N.cg.Cb > 65535 || !al16(out)) return LRS_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_concat_fwd4, dim3((unsigned)((q + 255) / 256), (unsigned)(N.cg.Ca + N.cg.Cb)), dim3(256), 0, st,
                       net->tensor(N.d.in0, x), net->tensor(N.d.in1, x), N.cg, out);
    return LRS_OK;
}

int dipnet_forward(lrs_dipnet *net, const float *x, hipStream_t st, const FwdStep &fs) {
    int rc;
    if (net->n_sn && !fs.raw_first) {
        rc = sn_launch(net->table(), net->n_sn, net->max_w, net->gram(), net->f(net->sigma_off),
                       net->f(net->scale_off), net->ln_lambda, false, st);
        if (rc) return rc;
    }
    if (net->n_prep && !fs.raw_first) {   // W / scale and the bf16 planes of every conv, one launch
        hipLaunchKernelGGL(k_conv_prep, dim3(kPrepWg, net->n_prep), dim3(256), 0, st, net->prep(), net->f(net->scale_off),
                           fs.begin ? net->loss_acc() : nullptr, net->step());
        LRS_CHECK_LAUNCH();
    }
    for (size_t i = 0; i < net->nodes.size(); ++i) {
        const auto &N = net->nodes[i];
        if (fs.raw_first && i == 1) {   // every later node may read the side stream's planes / W / scale
            const hipError_t e = hipStreamWaitEvent(st, net->ev_prep, 0);
            if (e != hipSuccess) return (int)e;
        }
        if (has_conv(N)) rc = conv_fwd_node(net, i, x, st, fs);
        else if (N.d.kind == LRS_NODE_BN) rc = bn_fwd_node(net, N, x, st);
        else rc = concat_fwd_node(net, N, x, st);
        if (rc) return rc;
    }
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// ---- backward ---------------------------------------------------------------------------------
// the early-stopping update of this step's output, run beside the backward (dipnet_step)
// (cr: the interior of a framed output, lrs_dipnet_set_frame; NULL without a frame)
struct EsJob { const float *out; int64_t N; float *ring; lrs_es_state *es; const EsCrop *cr; };

// What a training step adds to the backward; the defaults are a stand-alone backward, which starts from
// dL/d(output) in the last node's gradient buffer as Head::Generic does.
struct BwdStep {
    Head head = Head::Generic;   // != Generic: the loss head wrote the last node's gz and bias gradient;
                                 // Pw: its sums (k_head_reduce, k_head_loss) are still to run
    // the input conv's weight gradient may leave its split-K partials for k_adam to finish (AdamPend;
    // pend->part == nullptr when nothing is pending)
    AdamPend *pend = nullptr;
    const EsJob *es = nullptr;
};

// What the step gives to one stream, once: the first fork's side stream, else the main stream after the join.
struct SideOnce {
    bool head_sums;      // Head::Pw
    const EsJob *es;
    int take(lrs_dipnet *net, hipStream_t hs) {
        // the fused loss head's sums (PwHead): the bias gradient of the last conv (read by Adam only) and the
        // loss, on the side stream with the first weight gradient (or on the main one, where none forks)
        if (head_sums) {
            const auto &Lh = net->nodes.back();
            hipLaunchKernelGGL(k_head_reduce, dim3((unsigned)Lh.C), dim3(256), 0, hs, (const double *)net->hpart(), Lh.C,
                               net->head_nwg, net->head_gbias(Lh), net->closs());
            hipLaunchKernelGGL(k_head_loss, dim3(1), dim3(64), 0, hs, (const double *)net->closs(), Lh.C, net->loss_acc());
            head_sums = false;
        }
        // the ES update reads only the forward's output and its own ring: on the side stream with the first
        // weight gradients (its ring slot and window sums follow the previous step's there), joined before Adam
        if (!es) return LRS_OK;
        const EsJob *j = es;
        es = nullptr;
        return es_update(j->out, j->N, j->ring, j->es, hs, j->cr);
    }
};

// the backward's state as it walks the nodes from the last to the first
struct BwdWalk {
    std::vector<char> written;   // gradient buffers: the first contribution to a tensor writes, later ones accumulate
    // a small-map data gradient may leave dL/dy of the next node as split-K partials, finished by
    // that node's BatchNorm backward (launch_reduce_bn_bwd1; dy_part = the partials, dy_S their count)
    const float *dy_part = nullptr;
    int dy_S = 0;
    SideOnce once;
};

// split-K workgroup target of the weight gradients on the side stream: fewer splits would write fewer
// partials and hold fewer CUs beside the data-gradient chain (at most the 512 the workspace is sized for)
constexpr int kWgradSplitWg = 512;

// Weight gradient of conv node i on stream ws: reads dL/dz, the layer input and the scale only.
// scratch: its split-K partials (part2 on the side stream; part on the main one)
int weight_grad(lrs_dipnet *net, int i, const float *x, hipStream_t ws, float *scratch, int *wsplit_out = nullptr) {
    if (wsplit_out) *wsplit_out = 1;
    const int wt = ws == net->side ? kWgradSplitWg : 512;
    auto &N = net->nodes[i];
    const int t = N.d.in0;
    const float *gz = net->f(N.gz_off), *xin = net->tensor(t, x);
    float *gw = net->grads + N.w_off;
    const lrs_dipnet::ConvW cw = net->conv_w(N);
    const int P = (int)N.P;
    switch (N.plan.wgrad) {
    case Wgrad::Table:   // implicit col^T on k_conv_sm (SmWgrad), dW / scale in its epilogue
        return sm_launch(SmDense{gz, P, N.C},
                         SmWgrad{xin, N.g.Cin * N.g.Hs * N.g.Ws * 4, (int)N.Kc, N.g.k * N.g.k, P, N.g.Hs * N.g.Ws * 4,
                                 net->at<const int>(N.wtab_off)},
                         gw, nullptr, N.C, (int)N.Kc, P, 0, scratch, net->part_cap, ws, nullptr, cw.div, true);
    case Wgrad::Upc: return upc_wgrad(N.g, gz, xin, cw.div, N.C, gw, scratch, net->part_cap, ws, wt);
    case Wgrad::Im2colGemm: {   // the forward gathered inside k_conv_sm: the col for the weight gradient now
        const dim3 grid((unsigned)((P + 255) / 256), (unsigned)std::min<int64_t>(N.Kc, 65535));
        hipLaunchKernelGGL(k_im2col, grid, dim3(256), 0, ws, xin, N.g, net->f(N.col_off));
        break;
    }
    case Wgrad::Gemm: break;
    }
    // explicit: on the node's col buffer; implicit (no col buffer): col^T gathered from the input
    return conv_wgrad(N.g, gz, N.col_off >= 0 ? net->f(N.col_off) : xin, cw.div, N.C, gw, scratch, net->part_cap, ws,
                      N.col_off < 0, wsplit_out, wt);
}

// conv node j's weight gradient on the side stream, forked right after its BN backward (its dL/dz is
// complete by then).  Until round 5 a run of small maps forked every second conv (a fork cost the
// critical stream ~7 us with system-scope events); with the device-scope events (ensure_side) forking
// at every conv is faster at both sizes: 196^2 1.192 -> 1.189 ms, 36^2 0.584 -> 0.580 ms (3 interleaved
// rounds, profiles/r06/ab/fork_sets.txt).
int fork_wgrad(lrs_dipnet *net, int j, const float *x, hipStream_t st, SideOnce &once) {
    hipError_t e = hipEventRecord(net->ev_fork[j], st);
    if (e == hipSuccess) e = hipStreamWaitEvent(net->side, net->ev_fork[j], 0);
    if (e != hipSuccess) return (int)e;
    if (const int r = once.take(net, net->side)) return r;
    return weight_grad(net, j, x, net->side, net->f(net->part2_off));
}

int conv_bwd_node(lrs_dipnet *net, int i, const float *x, hipStream_t st, const BwdStep &bs, BwdWalk &wk) {
    auto &N = net->nodes[i];
    auto &written = wk.written;
    const NodePlan &pl = N.plan;
    const float *outp = net->f(N.out_off);
    float *gout = net->f(N.grad_off), *gz = net->f(N.gz_off);
    int rc;
    if (pl.tail != Tail::None) {
        // dL/dz on the conv's map: [BatchNorm backward on a ->] the tail's adjoint with the
        // activation's derivative
        const float *ga = gout, *a = outp;
        if (pl.tail_bn) {
            a = net->f(N.a_off);
            if ((rc = net->node_bn_bwd(N, a, LRS_ACT_NONE, net->f(N.ga_off), 0, st))) return rc;
            ga = net->f(N.ga_off);
        }
        rc = pl.tail == Tail::Up2Act ? up2_bwd(ga, a, N.C, N.g.Ho, N.g.Wo, N.d.act, gz, st)
                                     : dec_act_bwd_launch(ga, a, gz, (int64_t)N.C * N.P, N.d.act, st);
        if (rc) return rc;
    } else if (wk.dy_part) {
        launch_reduce_bn_bwd1(wk.dy_part, wk.dy_S, net->bn_bwd_args(N), st);
        wk.dy_part = nullptr;
    } else if (bs.head == Head::Generic || i + 1 < (int)net->nodes.size()) {   // else the loss head wrote gz and the bias gradient
        rc = net->node_bn_bwd(N, N.z_off >= 0 ? net->f(N.z_off) : outp, N.d.act, gz, 0, st);
        if (rc) return rc;
    }
    const int t = N.d.in0;
    const lrs_dipnet::ConvW cw = net->conv_w(N);
    float *gx = t > 0 ? net->f(net->nodes[t - 1].grad_off) : nullptr, *part = net->f(net->part_off);
    const __bf16 *wp = N.wpre_off >= 0 ? net->at<const __bf16>(N.wpre_off) : nullptr;
    // weight gradient on the side stream (reads gz, the layer input and the scale only)
    if (!(t == 0 && i == net->step_plan.first_conv)) {
        if ((rc = fork_wgrad(net, i, x, st, wk.once))) return rc;
    } else {
        // the first conv on the input, after which the main stream has no work left of its own (a
        // fork there only adds the event latency to the step's tail); it uses the main stream's
        // scratch, free by then, beside whatever the side stream still runs
        int wsplit = 1;
        const bool defer = bs.pend != nullptr;
        if ((rc = weight_grad(net, i, x, st, part, defer ? &wsplit : nullptr))) return rc;
        if (defer && wsplit > 1) *bs.pend = AdamPend{part, wsplit, N.w_off, (int64_t)N.C * N.Kc, cw.div, net->grads};
    }
    rc = LRS_OK;
    switch (N.plan.dgrad) {
    case Dgrad::None: break;
    case Dgrad::Upc:   // by output parity class over the extended source grid, then the clamp fold
        rc = upc_dgrad(N.g, gz, wp + wprep_elems(N.g, N.C, true).fwd, N.C, gx, net->f(net->dcol_off), part, net->part_cap,
                       st, written[t]);
        break;
    case Dgrad::Adjoint: {   // gx = the adjoint gather of dL/dz on k_conv_sm, one GEMM
        const auto &g = N.g;
        const int kk = g.k * g.k, Cop = r16(N.C);
        const SmPre la{wp + wprep_elems(g, N.C, false).fwd, (int64_t)g.Cin * kk * Cop, kk * Cop, g.Cin};
        // the next node (t - 1 = i - 1, this tensor's only other writer would come before it)
        // finishes the split-K sum inside its BN backward when that fits one workgroup
        const bool fuse_next = t == i && !written[t] && net->nodes[t - 1].plan.bn_bwd_fuse;
        int nsplit = 1;
        rc = sm_launch(la, SmAdj{gz, (int)(N.C * N.P * 4), g, N.C, Cop, net->at<const int4>(N.adj_off), nullptr}, gx,
                       nullptr, g.Cin, g.Hs * g.Ws, kk * Cop, written[t], part, net->part_cap, st,
                       fuse_next ? &nsplit : nullptr);
        if (fuse_next && nsplit > 1) {
            wk.dy_part = part;
            wk.dy_S = nsplit;
        }
        break;
    }
    case Dgrad::Gemm:
        rc = conv_dgrad(N.g, gz, cw.w, N.C, gx, !plain_unit(N.g) ? net->f(net->dcol_off) : nullptr, part, net->part_cap,
                        st, written[t], N.col_off < 0, wp);
        break;
    }
    if (rc) return rc;
    if (t > 0) written[t] = 1;
    return LRS_OK;
}

int bn_bwd_node(lrs_dipnet *net, const Node &N, const float *x, hipStream_t st, BwdWalk &wk) {
    const int t = N.d.in0;
    // (BN straight on the input: parameter grads only, dL/dx into the scratch dz)
    float *gx = t > 0 ? net->f(net->nodes[t - 1].grad_off) : net->f(net->dz_off);
    if (const int rc = net->node_bn_bwd(N, net->tensor(t, x), N.d.act, gx, t > 0 ? wk.written[t] : 0, st)) return rc;
    if (t > 0) wk.written[t] = 1;
    return LRS_OK;
}

int concat_bwd_node(lrs_dipnet *net, const Node &N, hipStream_t st, BwdWalk &wk) {
    auto &written = wk.written;
    const float *gout = net->f(N.grad_off);
    const int ta = N.d.in0, tb = N.d.in1;
    float *ga = ta > 0 ? net->f(net->nodes[ta - 1].grad_off) : nullptr;
    float *gb = tb > 0 ? net->f(net->nodes[tb - 1].grad_off) : nullptr;
    const int64_t na = ga ? (int64_t)N.cg.Ca * N.cg.Ha * N.cg.Wa : 0;
    const int64_t nb = gb ? (int64_t)N.cg.Cb * N.cg.Hb * N.cg.Wb : 0;
    if (na + nb > 0) {
        const int acc_a = ta > 0 ? written[ta] : 0;
        // both inputs may be the same tensor: the b pass must then accumulate onto the a pass
        const int acc_b = tb > 0 ? (written[tb] || (tb == ta)) : 0;
        // a then b (the same order as one launch over both when ta == tb)
        const CatGeom &cg = N.cg;
        if (ga) {
            if (!al16(ga)) return LRS_E_UNSUPPORTED;
            const int q = cg.Ha * ((cg.Wa + 3) / 4);
            hipLaunchKernelGGL(k_concat_bwd4, dim3((unsigned)((q + 255) / 256), (unsigned)cg.Ca), dim3(256), 0, st, gout,
                               cg, ga, acc_a, 0);
        }
        if (gb) {
            if (!al16(gb)) return LRS_E_UNSUPPORTED;
            const int q = cg.Hb * ((cg.Wb + 3) / 4);
            hipLaunchKernelGGL(k_concat_bwd4, dim3((unsigned)((q + 255) / 256), (unsigned)cg.Cb), dim3(256), 0, st, gout,
                               cg, gb, (ta == tb && ga) ? 1 : acc_b, 1);
        }
    }
    if (ta > 0) written[ta] = 1;
    if (tb > 0) written[tb] = 1;
    return LRS_OK;
}

// Backward from dL/d(output) already in the last node's gradient buffer (or, after a loss head that is not
// Head::Generic, from that node's dL/dz): every parameter gradient into net->grads (the input gets none:
// the reference's DIP input needs no gradient).
int dipnet_backward(lrs_dipnet *net, const float *x, hipStream_t st, const BwdStep &bs) {
    int rc;
    const int n = (int)net->nodes.size();
    BwdWalk wk{std::vector<char>(n + 1, 0), nullptr, 0, SideOnce{bs.head == Head::Pw, bs.es}};
    wk.written[n] = 1;
    for (int i = n - 1; i >= 0; --i) {
        const auto &N = net->nodes[i];
        if (!wk.written[i + 1]) continue;   // output unused by the loss (cannot happen for a valid net)
        if (has_conv(N)) rc = conv_bwd_node(net, i, x, st, bs, wk);
        else if (N.d.kind == LRS_NODE_BN) rc = bn_bwd_node(net, N, x, st, wk);
        else rc = concat_bwd_node(net, N, st, wk);
        if (rc) return rc;
    }
    {   // join the side stream before anyone reads the weight gradients
        hipError_t e = hipEventRecord(net->ev_join, net->side);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, net->ev_join, 0);
        if (e != hipSuccess) return (int)e;
    }
    if ((rc = wk.once.take(net, st))) return rc;   // (only if no fork took them)
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// ---- the training step --------------------------------------------------------------------------
// The step head of the overlapped sigma (StepPlan::sn_overlap):
// the spectral-norm Grams here (alone they take 19 us at 196^2; on the side stream beside the
// first conv, 50), then the rest of the chain (Gram reduce, Lanczos) and the preparation of every
// conv but the first on the side stream beside the first conv, whose planes come from the raw
// weights here
// (the Gram reduce too: on the side stream beside the first conv it took 23 us instead of 6)
int sn_overlap_head(lrs_dipnet *net, hipStream_t st) {
    hipLaunchKernelGGL(k_sn_gram_head, dim3(kSnSplit, net->n_sn + kHeadPlaneRows), dim3(256), 0, st, net->table(), net->gram(),
                       net->n_sn, (const ConvPrep *)net->prep_head(), net->loss_acc(), net->step());
    hipLaunchKernelGGL(k_sn_gram_reduce, dim3(kSnPairs, net->n_sn), dim3(256), 0, st, net->table(), net->gram());
    hipError_t e = hipEventRecord(net->ev_head, st);
    if (e == hipSuccess) e = hipStreamWaitEvent(net->side, net->ev_head, 0);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_sn_sigma, dim3(net->n_sn), dim3(256), 0, net->side, net->table(), net->gram(),
                       net->f(net->sigma_off), net->f(net->scale_off), net->ln_lambda, (long long *)nullptr);
    // the first BatchNorm waits for the scale only, the second conv for the planes as well: 196^2 step
    // 1.185 -> 1.179 ms against one event after both (3 interleaved rounds,
    // profiles/r06/ab/split_event_and_es.txt)
    if ((e = hipEventRecord(net->ev_sigma, net->side)) != hipSuccess) return (int)e;
    if (net->n_prep)
        hipLaunchKernelGGL(k_conv_prep, dim3(kPrepWg, net->n_prep), dim3(256), 0, net->side, net->prep_side(),
                           net->f(net->scale_off), (double *)nullptr, net->step());
    if ((e = hipEventRecord(net->ev_prep, net->side)) != hipSuccess) return (int)e;
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// mstride: the mask's row stride (mask_stride: 0 for a [P] mask or none, P for a [C][P] one)
int dipnet_step(lrs_dipnet *net, const float *x, const float *target, const float *mask, int64_t mstride, float lr,
                float b1, float b2, float eps, lrs_es_state *es, float *ring, hipStream_t st) {
    const StepPlan &sp = net->step_plan;
    int rc;
    // (the side stream and ev_head / ev_sigma / ev_prep exist: dipnet_step only runs after ensure_side
    // returned LRS_OK)
    if (sp.sn_overlap && (rc = sn_overlap_head(net, st))) return rc;
    const auto &Lst = net->nodes.back();
    // the loss head in the last conv's epilogue (k_pw): gz, and per-workgroup sums for the bias gradient
    // and the loss, reduced in the backward on the side stream (k_mse_head's arithmetic per element)
    const PwHead hd{target, mask, mstride, net->f(Lst.gz_off), net->hpart(),
                    net->framed ? (float)(2.0 / (double)net->n_mean())
                                : (float)(2.0 / ((double)Lst.C * (double)Lst.P)),
                    &net->head_nwg};
    const Head head = step_head(net, target, mask, mstride);
    // the weight-preparation launch at the head of the forward also zeroes the loss accumulator
    // and advances Adam's step counter (read only by this step's k_adam); without one, a tiny launch
    rc = dipnet_forward(net, x, st, FwdStep{sp.begin_in_prep, sp.sn_overlap, head == Head::Pw ? &hd : nullptr});
    if (rc) return rc;
    const float *out = net->f(Lst.out_off);
    if (!sp.begin_in_prep) hipLaunchKernelGGL(k_step_begin, dim3(1), dim3(64), 0, st, net->loss_acc(), net->step());
    rc = LRS_OK;
    if (head == Head::Mse)
        rc = mse_head(net, out, target, mask, mstride, st);
    else if (head == Head::Generic)
        rc = masked_mse(out, target, mask, mstride ? Lst.C : 1, Lst.C, Lst.P, net->n_mean(), net->f(Lst.grad_off),
                        net->loss_acc(), st);
    if (rc) return rc;
    // the input conv's weight-gradient split-K sum is finished inside Adam (one launch less on the
    // step's tail)
    AdamPend pw{};
    // (the early-stopping ring holds the interior of a framed output only: what the frame holds is
    // constrained by nothing and must not drive the stop)
    const EsCrop crop{net->fr_top, net->fr_left, net->fr_H, net->fr_W, Lst.H, Lst.W};
    const EsJob esj{out, net->n_mean(), ring, es, net->framed ? &crop : nullptr};
    rc = dipnet_backward(net, x, st, BwdStep{head, &pw, es ? &esj : nullptr});
    if (rc) return rc;
    hipLaunchKernelGGL(k_adam, dim3(ew_blocks((net->n_params + 3) / 4, 8192)), dim3(kEw), 0, st, net->params,
                       (const float *)net->grads, net->am, net->av, net->n_params, (const int *)net->step(), lr, b1, b2,
                       eps, pw);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// The side streams and the fork/join events are created on the first training call that needs
// them (outside any capture), so that creating a net and querying its layout needs no device.
// The side stream takes the priority of the calling stream, so a caller that trains the net on a
// high-priority stream (LrsPnPConfig.lowrank_priority) gets its weight gradients placed with the
// same priority.  One side stream is kept per priority seen (at most two in practice), so a call
// on a stream of another priority only selects a different one: no host synchronisation and no
// graph drop (a captured graph holds its own nodes, not the stream).
int ensure_side(lrs_dipnet *net, hipStream_t st) {
    int prio = 0;
    hipError_t e = hipStreamGetPriority(st, &prio);
    if (e != hipSuccess) return (int)e;
    for (auto &ps : net->sides)
        if (ps.first == prio) {
            net->side = ps.second;
            return LRS_OK;
        }
    hipStream_t s = nullptr;
    e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio);
    if (e != hipSuccess) return (int)e;
    net->sides.emplace_back(prio, s);
    net->side = s;
    // The fork / join events only order kernels of this device against each other (nothing on the host
    // waits on them), so they are recorded with device-scope fences -- what a kernel boundary inside one
    // stream has -- instead of the default system-scope release, whose cache write-back the critical
    // stream paid at every fork (tools/micro/fork_cost: DESIGN.md §5).
    constexpr unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;
    for (hipEvent_t *ev : {&net->ev_join, &net->ev_head, &net->ev_sigma, &net->ev_prep})
        if (e == hipSuccess && !*ev) e = hipEventCreateWithFlags(ev, evf);
    for (size_t i = 0; i < net->ev_fork.size() && e == hipSuccess; ++i)
        if (!net->ev_fork[i]) e = hipEventCreateWithFlags(&net->ev_fork[i], evf);
    return (int)e;
}

void drop_graph(lrs_dipnet *net) {
    if (net->gexec) (void)hipGraphExecDestroy(net->gexec);
    if (net->graph) (void)hipGraphDestroy(net->graph);
    net->gexec = nullptr; net->graph = nullptr; net->have_key = false;
}

// One step captured from st and instantiated as the net's graph under key k (x ... ring, st: dipnet_step's)
int capture_step(lrs_dipnet *net, const lrs_dipnet::Key &k, const float *x, const float *target, const float *mask,
                 lrs_es_state *es, float *ring, hipStream_t st) {
    drop_graph(net);
    hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return (int)e;
    const int rc = dipnet_step(net, x, target, mask, k.mstride, k.lr, k.b1, k.b2, k.eps, es, ring, st);
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(st, &g);
    if (rc) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess) return (int)e;
    e = hipGraphInstantiate(&net->gexec, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(g);
        return (int)e;
    }
    net->graph = g;
    net->key = k;
    net->have_key = true;
    return LRS_OK;
}

}  // namespace
