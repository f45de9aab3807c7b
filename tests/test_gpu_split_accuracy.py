"""GPU: every launched split-bf16 product (csrc/lrs_split.h) against fp64, one product at a time.

Every case builds its operands on the CPU (tests/split_emu.py: the same generators tests/test_split_emu.py
proves teeth for), takes the tolerance from the CPU model -- 3 x the error of a sequential fp32 GEMM on the
same operands, in relative L2 and componentwise -- and never from the kernel, runs the kernel into
NaN-filled outputs, prints what it measured and asserts both metrics.  The f32-MFMA paths meet the same
bound.  DESIGN.md 8.1 holds the rule, the measured values and the paths left out.

Kernel and loader pair each conv case reaches (dip_launch.h conv_fwd / conv_wgrad / conv_dgrad, dipnet_plan.h;
the kernels: dip_gemm.h k_gemm_s3 and its loaders, dip_pw.h k_pw, dip_dgrad.h the fold and border kernels,
dip_sm.h k_conv_sm):
  conv primitives, col == NULL (lrs_conv2d_fwd_f32 / lrs_conv2d_bwd_x_f32):
    s3_reflect   3x3 reflection, stride 1, 19 x 21 (ragged 128-tiles).  fwd k_gemm_s3<LdPre, LdFwdTM>;
                 dgrad <LdPre, LdDgradTM> over the padded domain + k_fold_pad; wgrad <LdDense, LdWgradTM>
    s3_up3       upsampled 3x3: fwd LdFwdTM through the x2 map; dgrad upsample_dgrad 0: LdDgradTM + fold,
                 1: the 4x4 stride-2 effective conv (LdFwdTM) + k_up_border_*; wgrad LdWgradTM.  16 output
                 channels: a source pixel is read through 36 (output, tap) pairs, 36 x 16 = 576
    s3_up2       upsampled 2x2 unpadded: the 3x3 effective kernel when upsample_dgrad = 1
    s3_stride2   3x3 stride 2, zero pad: the data gradient is not stride 1, so it runs W^T gz on k_gemm64
                 (f32 MFMA: M = 288, N = 121 is 3 128-tiles, under the 64 the split-bf16 GEMM needs) + k_col2im; held to the same bound
    s3_dense_tn  the same at 108^2 -> 54^2: 3 x 23 = 69 128-tiles, so that GEMM is k_gemm_s3<LdDense<false>,
                 LdDense<false>>.  Weight gradient left out: 2916 pixels of inner length
    s3_dense_nn  1x1 with 260 > 256 output channels (no k_pw): k_gemm_s3<LdDense<true>, LdDense<false>>, 66
                 tiles.  Forward only: its data gradient is 22 tiles of k_gemm64, its weight gradient 2704 long
    pw_MxN       1x1 on k_pw<M, N>: M = ceil(cout / 64) row blocks forward, ceil(cin / 64) in the data
                 gradient; the weight gradient is k_gemm_s3<LdDense<true>, LdDense<true>> with split-K.
                 pw_4x5 needs 32768 < pixels <= 40960 (196^2): forward and data gradient only
  network engine (a two-node lrs_dipnet: an identity 1x1, then the conv; its input, output, dL/dx and dW
  read back through lrs_dipnet_node_buffer / the gradient buffer):
    sm_table     3x3 on a 9 x 11 map: k_conv_sm<SmFwd, SmPre>, <SmAdj, SmPre>, <SmWgrad, SmDense> (<= 200 pixels)
    sm_split     the same on 19 x 21: the weight gradient is k_im2col + k_gemm64 there
    upc          upsampled 3x3 with >= 1024 output pixels: k_gemm_s3<LdPre, LdUpFwdTM>, <LdPre, LdUpDgradTM> +
                 clamp fold.  <LdGzCls, LdWgradCls> is left out: its inner length is the >= 1024 output pixels
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import split_emu as E  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lrspnp import _lib
    return _lib.device_lib()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def run_primitive(L, case, direction, tensors, precision, ud):
    """split-bf16: the implicit calls (col == NULL); f32: the explicit ones (col given) with LRS_DIP_F32.  A
    1x1 conv has no col, but col == NULL would send its forward to k_pw whatever the precision: the f32 run
    passes a one-float col, which the library never touches, and so reaches k_gemm / k_gemm64."""
    from lrspnp import _lib
    cin, cout, H, W, k, stride, pad, pm, up = case
    xd, wd, bd, gyd = (t.cuda().contiguous() for t in tensors)
    opts = ctypes.byref(_lib.dip_opts(precision, ud))
    nws = L.lrs_conv2d_workspace(cin, H, W, cout, k, stride, pad, up, opts)
    ws = torch.empty(nws // 4 + 1, device="cuda")
    ncol = L.lrs_conv2d_col_size(cin, H, W, k, stride, pad, up)
    col = torch.empty(max(ncol, 1), device="cuda") if precision == 0 else None
    geo = (cin, H, W, cout, k, stride, pad, pm, up)
    if direction == "fwd" or (precision == 0 and ncol):     # the explicit backward reads the forward's col
        y = nan(*gyd.shape)
        assert L.lrs_conv2d_fwd_f32(P(xd), cin, H, W, P(wd), P(bd), cout, k, stride, pad, pm, up,
                                    P(col), P(y), opts, P(ws), nws, S()) == 0
        if direction == "fwd":
            return y.cpu()
    div = torch.ones(1, device="cuda")                      # w_div = 1: exact
    gx, gw = nan(*xd.shape), nan(*wd.shape)
    if precision == 0:
        assert L.lrs_conv2d_bwd_f32(P(gyd), P(col) if ncol else P(xd), P(wd), P(div), *geo, P(gx), P(gw), opts, P(ws),
                                    nws, S()) == 0
    else:
        assert L.lrs_conv2d_bwd_x_f32(P(gyd), P(xd), P(wd), P(div), *geo, P(gx), P(gw), opts, P(ws), nws, S()) == 0
    return (gx if direction == "dgrad" else gw).cpu()


def run_engine(case, direction, tensors, precision, ud):
    """The conv as node 1 of a lrs_dipnet behind an identity 1x1 (node 0 gives it a tensor that takes a
    gradient).  Returns the result and the input the conv really read (node 0's output)."""
    from lrspnp import dip
    cin, cout, H, W, k, stride, pad, pm, up = case
    x, w, b, gy = tensors
    nodes = [dip.DipNode(dip.NODE_CONV, 0, 0, cin, 1, 1, 0, 1, 0, dip.BN_NONE, dip.ACT_NONE, 0, 0),
             dip.DipNode(dip.NODE_CONV, 1, 0, cout, k, stride, pad, pm, up, dip.BN_NONE, dip.ACT_NONE, 0, 0)]
    net = dip.DipNet(nodes, cin, H, W, precision=precision, upsample_dgrad=ud)
    w0, b0, _, _ = net.param_views(0)
    w1, b1, _, _ = net.param_views(1)
    with torch.no_grad():
        w0.copy_(torch.eye(cin).view(cin, cin, 1, 1)); b0.zero_()
        w1.copy_(w); b1.copy_(b)
        net.grads.fill_(float("nan"))
    xd = x.cuda().contiguous()
    y = net.forward(xd).clone()
    xin = net.node_buffer(0, 0).cpu()
    if direction == "fwd":
        return y.cpu(), xin
    net.backward(xd, gy.cuda().contiguous())
    torch.cuda.synchronize()
    if direction == "dgrad":
        return net.node_buffer(0, 3).cpu(), xin
    return net.param_views(1, net.grads)[0].clone().cpu(), xin


def run_conv(L, name, direction, opset, precision, ud, scale=1.0):
    case, tensors, (A, B) = E.conv_operands(name, direction, opset, scale)
    if E.CONV_CASES[name][2]:
        out, xin = run_engine(case, direction, tensors, precision, ud)
        tensors = (xin,) + tensors[1:]
        A, B = E.conv_gemm(case, direction, *tensors)          # on the input the conv read
    else:
        out = run_primitive(L, case, direction, tensors, precision, ud)
    return out, A, B


def check(label, C, A, B, rows=False):
    ref = E.reference(A, B)
    tol_l2, tol_cw, tol_row = E.tolerances(A, B, ref)
    C = torch.as_tensor(C).reshape(ref[0].shape)
    assert torch.isfinite(C).all(), f"{label}: output not written everywhere"
    l2, cw = E.metrics(C, A, B, ref)
    msg = f"{label}: rel L2 {l2:.3e} (tol {tol_l2:.3e}), componentwise {cw:.3e} (tol {tol_cw:.3e})"
    r = None
    if rows:
        r = float(E.row_rel(C, A, B, ref).max())
        msg += f", worst row {r:.3e} (tol {tol_row:.3e})"
    print(msg)
    assert l2 <= tol_l2 and cw <= tol_cw, msg
    if rows:
        assert r <= tol_row, msg


@pytest.fixture(params=[1, 0], ids=["split_bf16", "f32"])
def precision(request):
    return request.param


def _uds(name, direction):
    """Both values of upsample_dgrad where it changes anything: an upsampled conv's data gradient."""
    return (0, 1) if direction == "dgrad" and E.CONV_CASES[name][0][8] else (0,)


@pytest.mark.parametrize("name,direction,opset,ud",
                         [(n, dr, o, u) for n, dr, o in E.conv_products() for u in _uds(n, dr)])
def test_conv_product(L, name, direction, opset, precision, ud):
    out, A, B = run_conv(L, name, direction, opset, precision, ud)
    check(f"{name} {direction} ({opset}, {'split-bf16' if precision else 'f32'}, upsample_dgrad {ud})", out, A, B,
          rows=opset == "rowscale")


@pytest.mark.parametrize("name,direction,ud", [(n, dr, u) for n, (c, dirs, _) in E.CONV_CASES.items() for dr in dirs
                                               for u in _uds(n, dr)])
def test_conv_scaling_is_bitwise(L, name, direction, ud):
    """Set (e): A times 2^20 and 2^-20 with a zero bias scales the output bit for bit (the split, every
    product and every fp32 sum commute with a power of two while nothing under- or overflows)."""
    base = run_conv(L, name, direction, "meta", 1, ud)[0]
    assert torch.isfinite(base).all()
    for s in (2.0 ** 20, 2.0 ** -20):
        out = run_conv(L, name, direction, "meta", 1, ud, scale=s)[0]
        assert torch.equal(out, base * s), f"{name} {direction} x {s}"


def d(a):
    return torch.as_tensor(a).contiguous().cuda()


@pytest.mark.parametrize("nb,K,opset", E.dict_products())
def test_dict_stats_product(L, nb, K, opset):
    """k_dl_gemm (dictlearn.hip, its own staging of the planes) through ops.dict_stats: H = coefs^T coefs."""
    from lrspnp import ops
    coefs = E.dict_coefs(nb, K, opset)
    ws = ops.dict_workspace(16, 16, K, nb, "cuda")
    ws.view(torch.float32).fill_(float("nan"))
    H, _ = ops.dict_stats(d(coefs), H=nan(K, K), ws=ws)
    A, B = E.dict_gemm(coefs)
    check(f"dict_stats ({nb}, {K}) ({opset})", H.cpu(), A, B)


def _ista_args(nb):
    return torch.ones(nb, device="cuda"), torch.zeros(nb, dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("opset", E.ISTA_OPSETS)
def test_ista_one_step(L, opset, precision):
    """k_ista_b3 (split-bf16) / k_ista_res (f32): one soft-threshold iteration from x = 0 with T = 0 and
    alpha = 1, so coefs = (obs .* Yb) D is one product and phi = coefs D^T a second (checked on the coefs the
    kernel returned)."""
    from lrspnp import ops
    Yb, obs, D = E.ista_inputs(opset)
    alpha, thr = _ista_args(E.ISTA_NB)
    phi, coefs = ops.ista(d(Yb), d(obs), d(D), E.ISTA_N, alpha, thr, 1, ops.PROX_SOFT, phi=nan(E.ISTA_NB, E.ISTA_N),
                          coefs=nan(E.ISTA_NB, E.ISTA_K), want_coefs=True, precision=precision)
    tag = f"({opset}, {'split-bf16' if precision else 'f32'})"
    check(f"ista coefs {tag}", coefs.cpu(), *E.ista_gemm_coefs(Yb, obs, D))
    check(f"ista phi {tag}", phi.cpu(), *E.ista_gemm_phi(coefs.cpu(), D))


@pytest.mark.parametrize("opset", E.ISTA_OPSETS)
def test_ista_nlm_phi(L, opset):
    """k_ista_ln2 (the NLM prox on the split-bf16 products): its coefs pass through the NLM filter, so only
    the second product, phi = coefs D^T, is one product of known operands."""
    from lrspnp import ops
    Yb, obs, D = E.ista_inputs(opset)
    alpha = torch.ones(E.ISTA_NB, device="cuda")
    thr = torch.full((E.ISTA_NB,), E.ISTA_NLM_H, dtype=torch.float64, device="cuda")
    phi, coefs = ops.ista(d(Yb), d(obs), d(D), E.ISTA_N, alpha, thr, 1, ops.PROX_NLM, phi=nan(E.ISTA_NB, E.ISTA_N),
                          coefs=nan(E.ISTA_NB, E.ISTA_K), want_coefs=True)
    assert coefs.abs().sum() > 0
    check(f"ista NLM phi ({opset})", phi.cpu(), *E.ista_gemm_phi(coefs.cpu(), D))


@pytest.mark.parametrize("opset", E.ISTA_OPSETS)
def test_ista_pat_one_step(L, opset):
    """lrs_ista_pat_f32 (f32 MFMA): b = D^T (obs .* y) and phi = D x from x = 0; three shared patterns."""
    from lrspnp import ops
    Y2, obs2, pats, pat, D = E.ista_pat_inputs(opset)
    npat = E.ISTA_NPAT
    alpha, thr = _ista_args(E.ISTA_NB)
    plan, nt = ops.ista_pat_plan(pat, npat)
    ws = ops.ista_pat_prepare(d(D), d(pats), E.ISTA_N)
    phi, coefs = ops.ista_pat(d(Y2), d(pats), d(plan), nt, E.ISTA_K, E.ISTA_N, alpha, thr, 1, ws, ops.PROX_SOFT,
                              phi=nan(E.ISTA_NB, E.ISTA_N), coefs=nan(E.ISTA_NB, E.ISTA_K), want_coefs=True)
    check(f"ista_pat coefs ({opset})", coefs.cpu(), *E.ista_gemm_coefs(Y2, obs2, D))
    check(f"ista_pat phi ({opset})", phi.cpu(), *E.ista_gemm_phi(coefs.cpu(), D))
