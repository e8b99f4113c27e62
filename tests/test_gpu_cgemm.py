"""The bf16 conv-GEMM path (csrc/vae_cgemm.hpp) through the C ABI, against an exact emulation.

bf16 mode rounds each operand to bf16 once (stored activations, the transformed operand on its
way into LDS, the weight copy) and accumulates in fp32.  The reference here applies the same
roundings in torch (transform in fp32 -> bf16, weights -> bf16) and then computes the conv in
fp64, so the only differences left are the fp32 summation order and the final bf16 rounding of
the output: max-abs error <= 6e-3 of the output's max (bf16 has 8 significant bits, 2^-8 =
3.9e-3), per-channel sums <= 1e-3.  That is ~3x tighter than the generic bf16 bar of
tests/test_gpu_ops.py and pins the new kernel's indexing (taps, phases, tiles, split-K).

Shapes cover every tile the planner picks (32x32 .. 128x128), split-K, the sub-pixel phases of
k3 s2 p1 op1 and k4 s2 p1 transposed convs, stride-1 data gradients, 8-channel (padded RGB)
operands, and both sources of the swapped-axes weights (caller's wt_t / built in the
workspace)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from gpu_util import give_workspace

pytestmark = pytest.mark.gpu

SLOPE = 0.01
OUT_TOL = 6e-3


def _L():
    from vae_amd import _lib as L
    return L


def bf(t):
    return t.to(torch.bfloat16).float()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to("cuda", torch.bfloat16)


def nchw(t):
    return t.float().permute(0, 3, 1, 2).contiguous().cpu()


def relmax(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


class Xf:
    """A transform descriptor with a caller-made coefficient table (what vae_bn_finalize
    writes) plus the dummy statistics pointers the ABI validates."""

    def __init__(self, L, kind, C, table=None, aux=None):
        self.keep = [torch.zeros(4 * C, device="cuda")]
        d = self.keep[0]
        self.x = L.Xform(kind=kind, channels=C, slope=SLOPE, count=1.0, eps=1e-5, momentum=0.1)
        if kind in (L.X_BN_ACT, L.X_BN_DY):
            self.x.sum = self.x.sumsq = self.x.gamma = self.x.beta = d.data_ptr()
            self.x.dgamma = self.x.dbeta = d.data_ptr()
            t = table.contiguous().float().cuda()
            self.keep.append(t)
            self.x.table = t.data_ptr()
        if aux is not None:
            self.x.aux = aux.data_ptr()


def bn_act_table(C, g):
    a = 0.5 + torch.rand(C, generator=g)
    b = torch.rand(C, generator=g) - 0.5
    return a, b


def emulate_act(kind, L, y, a=None, b=None):
    """The kernel's A operand in NCHW fp32: transform in fp32 then round to bf16."""
    if kind == L.X_NONE:
        return y
    if kind == L.X_ACT:
        return bf(F.leaky_relu(y, SLOPE))
    return bf(F.leaky_relu(y * a.view(1, -1, 1, 1) + b.view(1, -1, 1, 1), SLOPE))


def run_fwd(transposed, N, cin, cout, hw, stride, R, pad, kind, split=0, give_wt_t=False, seed=0):
    L = _L()
    g = torch.Generator().manual_seed(seed)
    y = bf(torch.randn(N, cin, hw, hw, generator=g))
    a_t, b_t = bn_act_table(cin, g)
    if transposed:
        w = bf(torch.randn(cin, cout, R, R, generator=g) * 0.1)
        P = (hw - 1) * stride - 2 * pad + R + (stride - 1 if R == 3 else 0)
    else:
        w = bf(torch.randn(cout, cin, R, R, generator=g) * 0.1)
        P = (hw + 2 * pad - R) // stride + 1
    bias = torch.randn(cout, generator=g) * 0.1
    act = emulate_act(kind, L, y, a_t, b_t).double()
    if transposed:
        acc = F.conv_transpose2d(act, w.double(), None, stride=stride, padding=pad,
                                 output_padding=(stride - 1 if R == 3 else 0))
    else:
        acc = F.conv2d(act, w.double(), None, stride=stride, padding=pad)
    ref = acc + bias.double().view(1, -1, 1, 1)
    yd = nhwc(y)
    wd = w.permute(0, 2, 3, 1).contiguous().to("cuda", torch.bfloat16)
    out = torch.empty(N, P, P, cout, device="cuda", dtype=torch.bfloat16)
    sums = torch.zeros(2 * cout, device="cuda")
    bd = bias.cuda()
    xf = Xf(L, kind, cin, table=torch.cat([a_t, b_t, torch.zeros(2 * cin)]) if kind == L.X_BN_ACT else None)
    a = L.ConvArgs(dtype=L.BF16, n=N, h=hw, w=hw, c=cin, k=cout, p=P, q=P, r=R, stride=stride, pad=pad)
    a.x = yd.data_ptr(); a.x_xf = xf.x; a.wt = wd.data_ptr(); a.bias = bd.data_ptr(); a.y = out.data_ptr()
    a.y_sum = sums.data_ptr(); a.y_sumsq = sums.data_ptr() + 4 * cout
    a.split_k = split
    if give_wt_t:
        wt = w.permute(1, 2, 3, 0).contiguous().to("cuda", torch.bfloat16)     # [cout][r][s][cin]
        a.wt_t = wt.data_ptr()
    ws = give_workspace(a, "vae_convT2d_fwd" if transposed else "vae_conv2d_fwd")
    L.call("vae_convT2d_fwd" if transposed else "vae_conv2d_fwd", ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    e_out, e_s1 = relmax(nchw(out), ref), relmax(sums[:cout].cpu(), acc.sum((0, 2, 3)))
    e_s2 = relmax(sums[cout:].cpu(), (acc * acc).sum((0, 2, 3)))
    print(f"fwd {'convT' if transposed else 'conv'} N={N} {cin}->{cout} hw={hw} R={R} kind={kind}: "
          f"out {e_out:.2e} (bar {OUT_TOL}), sum {e_s1:.2e}, sumsq {e_s2:.2e} (bar 1e-3)")
    assert e_out < OUT_TOL
    assert e_s1 < 1e-3
    assert e_s2 < 1e-3


FWD = [  # N, cin, cout, hw, stride, R, pad
    (8, 32, 64, 32, 2, 3, 1),
    (4, 64, 128, 16, 2, 3, 1),
    (4, 128, 256, 8, 2, 3, 1),
    (2, 256, 512, 4, 2, 3, 1),          # deep K, few rows: split-K
    (16, 256, 256, 16, 1, 3, 1),        # VQ-VAE residual 3x3 (large tiles)
    (8, 8, 32, 64, 2, 3, 1),            # padded-RGB first layer
    (8, 128, 256, 32, 2, 4, 1),         # VQ-VAE encoder k4 s2
]


@pytest.mark.parametrize("shape", FWD)
@pytest.mark.parametrize("kind", ["none", "act", "bn_act"])
def test_cgemm_conv2d_fwd(shape, kind):
    L = _L()
    k = {"none": L.X_NONE, "act": L.X_ACT, "bn_act": L.X_BN_ACT}[kind]
    run_fwd(False, *shape, k)


def test_cgemm_conv2d_fwd_split():
    L = _L()
    run_fwd(False, 4, 64, 128, 16, 2, 3, 1, L.X_BN_ACT, split=3)


CONVT = [  # N, cin, cout, hw, stride, R, pad
    (8, 512, 256, 2, 2, 3, 1),
    (8, 256, 128, 4, 2, 3, 1),
    (8, 64, 32, 16, 2, 3, 1),
    (8, 32, 32, 32, 2, 3, 1),
    (8, 256, 128, 16, 2, 4, 1),         # VQ-VAE decoder k4 s2
]


@pytest.mark.parametrize("shape", CONVT)
@pytest.mark.parametrize("give_wt_t", [False, True])
def test_cgemm_convT2d_fwd(shape, give_wt_t):
    L = _L()
    run_fwd(True, *shape, L.X_BN_ACT if shape[5] == 3 else L.X_ACT, give_wt_t=give_wt_t)


def run_dgrad(transposed, N, cin, cout, hw, stride, R, pad, dy_kind, epi_kind, give_wt_t=False, seed=1, odd_aux=False):
    """dx of conv2d / conv_transpose2d: dy (optionally through BN-backward on load), then the
    epilogue's activation backward (+ Σg, Σg·x̂ for a BatchNorm-followed input).  odd_aux: the
    stored pre-activation of x starts one element past a 16-byte boundary."""
    L = _L()
    g = torch.Generator().manual_seed(seed)
    if transposed:
        w = bf(torch.randn(cin, cout, R, R, generator=g) * 0.1)
        P = (hw - 1) * stride - 2 * pad + R + (stride - 1 if R == 3 else 0)
    else:
        w = bf(torch.randn(cout, cin, R, R, generator=g) * 0.1)
        P = (hw + 2 * pad - R) // stride + 1
    gy = bf(torch.randn(N, cout, P, P, generator=g))             # stored gradient
    yst = bf(torch.randn(N, cout, P, P, generator=g))            # stored pre-activation of the output
    A, Bc, Cc = (0.5 + torch.rand(cout, generator=g), torch.rand(cout, generator=g) - 0.5,
                 (torch.rand(cout, generator=g) - 0.5) * 0.1)
    if dy_kind == L.X_BN_DY:
        dyp = bf(A.view(1, -1, 1, 1) * gy + Bc.view(1, -1, 1, 1) * yst + Cc.view(1, -1, 1, 1))
    else:
        dyp = gy
    x0 = torch.zeros(N, cin, hw, hw, dtype=torch.float64, requires_grad=True)
    if transposed:
        out = F.conv_transpose2d(x0, w.double(), None, stride=stride, padding=pad,
                                 output_padding=(stride - 1 if R == 3 else 0))
    else:
        out = F.conv2d(x0, w.double(), None, stride=stride, padding=pad)
    out.backward(dyp.double())
    v = x0.grad
    xst = bf(torch.randn(N, cin, hw, hw, generator=g))           # stored pre-activation of x
    ea, eb = bn_act_table(cin, g)
    ep, eq = 0.5 + torch.rand(cin, generator=g), torch.rand(cin, generator=g) - 0.5
    if epi_kind == L.X_BN_ACT:
        z = xst * ea.view(1, -1, 1, 1) + eb.view(1, -1, 1, 1)
        gout = torch.where(z > 0, v, v * SLOPE)
        s1 = gout.sum((0, 2, 3))
        s2 = (gout * (xst * ep.view(1, -1, 1, 1) + eq.view(1, -1, 1, 1))).sum((0, 2, 3))
    elif epi_kind == L.X_ACT:
        gout = torch.where(xst > 0, v, v * SLOPE)
    else:
        gout = v
    gyd, ystd, xstd = nhwc(gy), nhwc(yst), nhwc(xst)
    if odd_aux:
        hold = torch.zeros(xstd.numel() + 8, device="cuda", dtype=torch.bfloat16)
        hold[1:1 + xstd.numel()].copy_(xstd.flatten())
        xstd = hold[1:1 + xstd.numel()]
        assert xstd.data_ptr() % 16 == 2
    wd = w.permute(0, 2, 3, 1).contiguous().to("cuda", torch.bfloat16)
    dx = torch.empty(N, hw, hw, cin, device="cuda", dtype=torch.bfloat16)
    dgam = torch.zeros(cin, device="cuda"); dbet = torch.zeros(cin, device="cuda")
    dyx = Xf(L, dy_kind, cout, table=torch.cat([A, Bc, Cc]) if dy_kind == L.X_BN_DY else None,
             aux=ystd if dy_kind == L.X_BN_DY else None)
    epx = Xf(L, epi_kind, cin, table=torch.cat([ea, eb, ep, eq]) if epi_kind == L.X_BN_ACT else None,
             aux=xstd if epi_kind != L.X_NONE else None)
    a = L.ConvArgs(dtype=L.BF16, n=N, h=hw, w=hw, c=cin, k=cout, p=P, q=P, r=R, stride=stride, pad=pad)
    a.dy = gyd.data_ptr(); a.dy_xf = dyx.x; a.wt = wd.data_ptr(); a.dx = dx.data_ptr(); a.dx_epi = epx.x
    a.dx_dgamma = dgam.data_ptr(); a.dx_dbeta = dbet.data_ptr()
    if give_wt_t:
        wt = w.permute(1, 2, 3, 0).contiguous().to("cuda", torch.bfloat16)
        a.wt_t = wt.data_ptr()
    ws = give_workspace(a, "vae_convT2d_bwd_data" if transposed else "vae_conv2d_bwd_data")
    L.call("vae_convT2d_bwd_data" if transposed else "vae_conv2d_bwd_data", ctypes.byref(a),
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    e_dx = relmax(nchw(dx), gout)
    msg = f"dgrad {'convT' if transposed else 'conv'} N={N} {cin}->{cout} hw={hw} R={R}: dx {e_dx:.2e} (bar {OUT_TOL})"
    if epi_kind == L.X_BN_ACT:
        e_s1, e_s2 = relmax(dbet.cpu(), s1), relmax(dgam.cpu(), s2)
        msg += f", sum g {e_s1:.2e}, sum g*xhat {e_s2:.2e} (bar 1e-3)"
    print(msg)
    assert e_dx < OUT_TOL
    if epi_kind == L.X_BN_ACT:
        assert e_s1 < 1e-3
        assert e_s2 < 1e-3


DGRAD = [  # N, cin, cout, hw (input of the conv), stride, R, pad
    (8, 32, 64, 16, 2, 3, 1),
    (8, 128, 256, 8, 2, 3, 1),
    (8, 256, 512, 4, 2, 3, 1),
    (8, 256, 256, 16, 1, 3, 1),          # VQ-VAE residual 3x3 data gradient
    (8, 128, 256, 32, 2, 4, 1),          # VQ-VAE encoder k4 s2
]


@pytest.mark.parametrize("shape", DGRAD)
@pytest.mark.parametrize("give_wt_t", [False, True])
def test_cgemm_conv2d_bwd_data(shape, give_wt_t):
    L = _L()
    run_dgrad(False, *shape, L.X_BN_DY, L.X_BN_ACT, give_wt_t=give_wt_t)


@pytest.mark.parametrize("epi", ["none", "act"])
def test_cgemm_conv2d_bwd_data_plain(epi):
    L = _L()
    run_dgrad(False, 8, 256, 256, 16, 1, 3, 1, L.X_NONE, L.X_NONE if epi == "none" else L.X_ACT)


def test_conv2d_bwd_data_stride1_flipped_weights():
    """The stride-1 data gradient the conv-GEMM refuses (here: a stored pre-activation that is not
    16-byte aligned), with a workspace: a forward conv of dy over the flipped weight copy staged at
    the workspace's end, on the generic kernel.  Two row tiles x one column tile, K = 144."""
    from gpu_util import launched
    L = _L()
    log = launched(lambda: run_dgrad(False, 2, 16, 16, 8, 1, 3, 1, L.X_NONE, L.X_ACT, odd_aux=True))
    assert "flip_weights_kernel" in log and "igemm_kernel" in log and "cgemm_kernel" not in log, log


# ---------------------------------------------------------------------------------------------
# The partial last batch of an epoch (the data path never drops it): N = 1, 7, 19 on the deep
# layers' 2x2 / 4x4 maps gives M = 4N / 16N rows that end inside a row tile (28 < 32; 76 = 64 + 12
# = 2*32 + 12; 16) — the masked rows of the forward statistics and of the E_BNBWD epilogue sums.
# Same references and bars as above; each case also asserts cgemm_kernel from the launch log.

def _ran(kernel, fn):
    from gpu_util import launched
    log = launched(fn)
    assert kernel in log, log


FWD_LAST = [(7, 256, 512, 4, 2, 3, 1), (19, 256, 512, 4, 2, 3, 1)]
CONVT_LAST = [(7, 512, 256, 2, 2, 3, 1), (19, 256, 128, 4, 2, 3, 1)]


@pytest.mark.parametrize("shape", FWD_LAST)
@pytest.mark.parametrize("kind", ["none", "act", "bn_act"])
def test_cgemm_conv2d_fwd_last_batch(shape, kind):
    L = _L()
    k = {"none": L.X_NONE, "act": L.X_ACT, "bn_act": L.X_BN_ACT}[kind]
    _ran("cgemm_kernel", lambda: run_fwd(False, *shape, k))


@pytest.mark.parametrize("shape", CONVT_LAST)
@pytest.mark.parametrize("give_wt_t", [False, True])
def test_cgemm_convT2d_fwd_last_batch(shape, give_wt_t):
    L = _L()
    _ran("cgemm_kernel", lambda: run_fwd(True, *shape, L.X_BN_ACT, give_wt_t=give_wt_t))


DGRAD_LAST = [(7, 256, 512, 4, 2, 3, 1),         # M = 112
              (1, 256, 512, 4, 2, 3, 1),         # M = 16
              (19, 128, 256, 8, 2, 3, 1)]
DGRAD_T_LAST = [(7, 512, 256, 2, 2, 3, 1),       # M = 28
                (19, 64, 32, 16, 2, 3, 1)]


@pytest.mark.parametrize("shape", DGRAD_LAST)
@pytest.mark.parametrize("give_wt_t", [False, True])
def test_cgemm_conv2d_bwd_data_last_batch(shape, give_wt_t):
    L = _L()
    _ran("cgemm_kernel", lambda: run_dgrad(False, *shape, L.X_BN_DY, L.X_BN_ACT, give_wt_t=give_wt_t))


@pytest.mark.parametrize("shape", DGRAD_T_LAST)
def test_cgemm_convT2d_bwd_data_last_batch(shape):
    L = _L()
    _ran("cgemm_kernel", lambda: run_dgrad(True, *shape, L.X_BN_DY, L.X_BN_ACT))


DGRAD_T = [  # N, cin, cout, hw (input of the transposed conv), stride, R, pad
    (8, 512, 256, 2, 2, 3, 1),
    (8, 64, 32, 16, 2, 3, 1),
    (8, 32, 32, 32, 2, 3, 1),
    (8, 256, 128, 16, 2, 4, 1),
]


@pytest.mark.parametrize("shape", DGRAD_T)
def test_cgemm_convT2d_bwd_data(shape):
    L = _L()
    run_dgrad(True, *shape, L.X_BN_DY if shape[5] == 3 else L.X_NONE, L.X_BN_ACT if shape[5] == 3 else L.X_ACT)


# ---------------------------------------------------------------------------------------------
# Weight gradients (csrc/vae_wgemm.hpp) with the BatchNorm coefficients built in-kernel from
# the statistics (no precomputed table: vae_common.hpp tab_build), plus the closed-form conv
# bias gradient and dL/dgamma, dL/dbeta published by the first workgroup.

class BN:
    """A stored pre-BN tensor with consistent statistics (sums over N*H*W, shift = the producing
    conv's bias) as the producing kernels leave them: one copy, or with reps > 1 spread over `reps`
    unequal replica rows `rstride` floats apart (default C; bn_ref.split_replicas, NaN between the
    rows), the dgamma / dbeta handed to xf() included."""

    def __init__(self, y, g, shift=None, reps=1, rstride=None):
        C = y.shape[1]
        self.reps, self.rstride, self.g = reps, (C if rstride is None else rstride), g
        self.y = y
        self.gamma = 0.7 + 0.6 * torch.rand(C, generator=g)
        self.beta = (torch.rand(C, generator=g) - 0.5) * 0.2
        self.shift = shift if shift is not None else torch.zeros(C)
        d = (y - self.shift.view(1, -1, 1, 1)).double()
        self.sum = d.sum((0, 2, 3)).float()
        self.sumsq = (d * d).sum((0, 2, 3)).float()
        self.count = y.numel() // C
        self.keep = []

    def xf(self, L, kind, aux_dev=None, dgamma=None, dbeta=None, dgamma_out=None, dbeta_out=None):
        C = self.gamma.numel()
        x = L.Xform(kind=kind, channels=C, slope=SLOPE, count=float(self.count), eps=1e-5, momentum=0.1)
        for name in ("sum", "sumsq", "shift", "gamma", "beta"):
            t = getattr(self, name).float()
            t = (self.spread(t) if name in ("sum", "sumsq") else t).cuda()
            self.keep.append(t)
            setattr(x, name, t.data_ptr())
        x.reps, x.rstride = self.reps, self.rstride
        if dgamma is not None:
            for name, t in (("dgamma", dgamma), ("dbeta", dbeta)):
                t = self.spread(t.float()).cuda()
                self.keep.append(t)
                setattr(x, name, t.data_ptr())
        if dgamma_out is not None:
            x.dgamma_out, x.dbeta_out = dgamma_out.data_ptr(), dbeta_out.data_ptr()
        if aux_dev is not None:
            x.aux = aux_dev.data_ptr()
        return x

    def spread(self, total):
        if self.reps <= 1:
            return total
        from bn_ref import split_replicas
        return split_replicas(total, self.reps, self.rstride, self.g).contiguous()

    def act(self, rnd=bf):
        z = F.batch_norm(self.y.double(), None, None, self.gamma.double(), self.beta.double(), True, 0.1, 1e-5)
        return rnd(F.leaky_relu(z, SLOPE).float())


def prep_wgrad(transposed, N, cin, cout, hw, stride, R, pad, x_kind, dy_kind, seed=3, fp32=False, odd_dy=False, reps=1):
    """One bf16 weight-gradient call's arguments (kernel-side operands) and its fp64 reference.
    fp32: the parity mode's call instead (fp32 operands, nothing rounded to bf16, every partial sum
    added in a fixed order: vae_conv_args.deterministic), against the same fp64 reference.
    odd_dy: the stored gradient starts 8 bytes past a 16-byte boundary.  reps: replicas of both
    BatchNorms' statistics (BN)."""
    L = _L()
    bf = (lambda t: t.float()) if fp32 else globals()["bf"]
    nhwc = (lambda t: t.permute(0, 2, 3, 1).contiguous().to("cuda", torch.float32)) if fp32 else globals()["nhwc"]
    g = torch.Generator().manual_seed(seed)
    if transposed:
        P = (hw - 1) * stride - 2 * pad + R + (stride - 1 if R == 3 else 0)
        wshape = (cin, cout, R, R)
    else:
        P = (hw + 2 * pad - R) // stride + 1
        wshape = (cout, cin, R, R)
    xst = bf(torch.randn(N, cin, hw, hw, generator=g) * 1.3 + 0.2)
    yst = bf(torch.randn(N, cout, P, P, generator=g) * 1.1 - 0.1)      # pre-BN output (BN_DY aux)
    gst = bf(torch.randn(N, cout, P, P, generator=g))                   # dL/dz of its BatchNorm
    bnx = BN(xst, g, reps=reps)
    bny = BN(yst, g, shift=torch.randn(cout, generator=g) * 0.1, reps=reps)
    # operands as the kernel forms them
    if x_kind == L.X_BN_ACT:
        act = bnx.act(bf)
    elif x_kind == L.X_ACT:
        act = bf(F.leaky_relu(xst, SLOPE))
    else:
        act = xst
    if dy_kind == L.X_BN_DY:
        yv = yst.double().requires_grad_(True)
        z = F.batch_norm(yv, None, None, bny.gamma.double(), bny.beta.double(), True, 0.1, 1e-5)
        z.backward(gst.double())
        dyp = bf(yv.grad.float())
        db_exact = yv.grad.sum((0, 2, 3))          # ~0: a train-mode BatchNorm's input gradient sums to 0
        xh = ((yst.double() - yst.double().mean((0, 2, 3), keepdim=True)) /
              torch.sqrt(yst.double().var((0, 2, 3), unbiased=False, keepdim=True) + 1e-5))
        dgam, dbet = (gst.double() * xh).sum((0, 2, 3)), gst.double().sum((0, 2, 3))
    else:
        dyp, dgam, dbet, db_exact = gst, None, None, None
    w0 = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    if transposed:
        out = F.conv_transpose2d(act.double(), w0, None, stride=stride, padding=pad,
                                 output_padding=(stride - 1 if R == 3 else 0))
    else:
        out = F.conv2d(act.double(), w0, None, stride=stride, padding=pad)
    out.backward(dyp.double())
    want = w0.grad.permute(0, 2, 3, 1)                                 # native [a][r][s][b]
    xd, yd, gd = nhwc(xst), nhwc(yst), nhwc(gst)
    if odd_dy:
        hold = torch.zeros(gd.numel() + 8, device="cuda", dtype=gd.dtype)
        hold[4:4 + gd.numel()].copy_(gd.flatten())
        gd = hold[4:4 + gd.numel()]
        assert gd.data_ptr() % 16 == 8
    dw = torch.zeros(want.shape, device="cuda")
    db = torch.zeros(cout, device="cuda")
    dgo = torch.zeros(cout, device="cuda"); dbo = torch.zeros(cout, device="cuda")
    a = L.ConvArgs(dtype=L.F32 if fp32 else L.BF16, n=N, h=hw, w=hw, c=cin, k=cout, p=P, q=P, r=R, stride=stride,
                   pad=pad, deterministic=1 if fp32 else 0)
    a.x = xd.data_ptr(); a.x_xf = bnx.xf(L, x_kind) if x_kind == L.X_BN_ACT else L.Xform(kind=x_kind, channels=cin, slope=SLOPE)
    a.dy = gd.data_ptr()
    if dy_kind == L.X_BN_DY:
        a.dy_xf = bny.xf(L, L.X_BN_DY, aux_dev=yd, dgamma=dgam, dbeta=dbet, dgamma_out=dgo, dbeta_out=dbo)
        a.db = db.data_ptr()
    a.dw = dw.data_ptr()
    fn = "vae_convT2d_bwd_filter" if transposed else "vae_conv2d_bwd_filter"
    return dict(a=a, fn=fn, want=want, dw=dw, db=db, dgo=dgo, dbo=dbo, db_exact=db_exact, dyp=dyp, dgam=dgam,
                dbet=dbet, keep=(xd, yd, gd, bnx, bny), R=R, untransformed=(x_kind == L.X_NONE and dy_kind == L.X_NONE))


def check_wgrad(w):
    """The call's dW (and closed-form bias / BN affine gradients) against the fp64 reference."""
    torch.cuda.synchronize()
    dw, want, R = w["dw"], w["want"], w["R"]
    e_dw = relmax(dw.cpu(), want)
    print(f"{w['fn']} dW {tuple(want.shape)}: {e_dw:.2e} (bar 2e-3)")
    assert e_dw < 2e-3
    if w["untransformed"]:
        # untransformed operands are exact bf16 in the fp64 reference: only fp32 accumulation order
        # separates the two, so the whole tensor must agree to ~1e-6 (a dropped or doubled K slice,
        # tap or row block shows here long before it moves the max-abs bar)
        d = dw.cpu().double() - want
        err = float(d.norm() / want.norm())
        if not err < 1e-4:
            per_tap = [float(d[:, r, s_].norm() / want[:, r, s_].norm()) for r in range(R) for s_ in range(R)]
            raise AssertionError(f"weight gradient rel-norm error {err:.3e}; per tap {per_tap}")
    if w["db_exact"] is not None:
        # closed form A*Σg + B*Σy + C*M (vaehip.h bn_args): exact up to fp32 cancellation
        e_db = float((w["db"].cpu().double() - w["db_exact"]).abs().max())
        b_db = 1e-6 * float(w["dyp"].double().abs().sum((0, 2, 3)).max())
        e_dg, e_dbt = relmax(w["dgo"].cpu(), w["dgam"]), relmax(w["dbo"].cpu(), w["dbet"])
        print(f"    bias grad {e_db:.2e} (bar {b_db:.2e}), dgamma {e_dg:.2e}, dbeta {e_dbt:.2e} (bar 1e-5)")
        assert e_db < b_db
        assert e_dg < 1e-5 and e_dbt < 1e-5


def run_wgrad(transposed, N, cin, cout, hw, stride, R, pad, x_kind, dy_kind, seed=3, odd_dy=False, reps=1):
    """One standalone bf16 weight-gradient call (its queried workspace given) against fp64."""
    L = _L()
    w = prep_wgrad(transposed, N, cin, cout, hw, stride, R, pad, x_kind, dy_kind, seed, odd_dy=odd_dy, reps=reps)
    a, fn = w["a"], w["fn"]
    ws = give_workspace(a, fn)           # 4 bytes when the plan takes none
    L.call(fn, ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    check_wgrad(w)


WGRAD = [  # N, cin, cout, hw (conv input), stride, R, pad
    (8, 32, 64, 32, 2, 3, 1),
    (8, 64, 128, 16, 2, 3, 1),
    (8, 256, 512, 4, 2, 3, 1),
    (8, 8, 32, 64, 2, 3, 1),             # padded-RGB first layer (x untransformed)
]


@pytest.mark.parametrize("shape", WGRAD)
def test_wgemm_conv2d_bn(shape):
    L = _L()
    run_wgrad(False, *shape, L.X_NONE if shape[1] == 8 else L.X_BN_ACT, L.X_BN_DY)


@pytest.mark.parametrize("transposed,shape,reps", [
    (False, WGRAD[1], 4),                 # 64 -> 128 channels, 4 replicas (a plan's count at 64): one-round build
    (True, (8, 128, 64, 8, 2, 3, 1), 4),  # WGRAD_T[1]
    (False, WGRAD[1], 32),                # reps·C = 2048 and 4096 > 1024: the plain loop, two rounds of replicas
])
def test_wgemm_bn_replicated_stats(transposed, shape, reps):
    """test_wgemm_conv2d_bn / test_wgemm_convT2d_bn with the statistics of both operands' BatchNorms in
    replicas (Σ, Σ² of x; Σ, Σ², Σg·x̂, Σg of y), also for the first workgroup's closed-form bias
    gradient and dgamma_out / dbeta_out."""
    L = _L()
    run_wgrad(transposed, *shape, L.X_BN_ACT, L.X_BN_DY, reps=reps)


def test_wgemm_conv2d_vq_shapes():
    L = _L()
    run_wgrad(False, 4, 256, 256, 16, 1, 3, 1, L.X_ACT, L.X_NONE)
    run_wgrad(False, 4, 128, 256, 32, 2, 4, 1, L.X_ACT, L.X_NONE)


WGRAD_T = [  # N, cin, cout, hw (convT input), stride, R, pad
    (8, 512, 256, 2, 2, 3, 1),
    (8, 128, 64, 8, 2, 3, 1),
    (8, 32, 32, 32, 2, 3, 1),
]


@pytest.mark.parametrize("shape", WGRAD_T)
def test_wgemm_convT2d_bn(shape):
    L = _L()
    run_wgrad(True, *shape, L.X_BN_ACT, L.X_BN_DY)


def test_conv2d_bwd_filter_tap_tile_kernel():
    """The 128 x 128 one-tap kernel (vae_wgrad.hpp) takes a bf16 weight gradient the weight-gradient
    GEMM refuses (here: a gradient tensor that is not 16-byte aligned) with at least 64 channels on
    both sides and 8192 output pixels: 8 x 32 x 32, 64 -> 64 (half a tile each way), one tile per
    tap, 32 K slices of 256 pixels."""
    L = _L()
    _ran("wgrad_bf16_kernel", lambda: run_wgrad(False, 8, 64, 64, 32, 1, 3, 1, L.X_ACT, L.X_NONE, odd_dy=True))


def test_wgemm_convT2d_vq_shape():
    L = _L()
    run_wgrad(True, 4, 256, 128, 16, 2, 4, 1, L.X_ACT, L.X_NONE)


# The pixel (K) tail of the weight gradients at a partial last batch: 4N = 28 pixels (less than one
# 32-pixel K-step) and 76 = 2*32 + 12 on the output side of the conv, on the input side of the
# transposed conv; 16N = 112 and 304 on the other operand.
@pytest.mark.parametrize("N", [7, 19])
def test_wgemm_conv2d_bn_last_batch(N):
    L = _L()
    _ran("wgemm", lambda: run_wgrad(False, N, 256, 512, 4, 2, 3, 1, L.X_BN_ACT, L.X_BN_DY))


@pytest.mark.parametrize("N", [7, 19])
def test_wgemm_convT2d_bn_last_batch(N):
    L = _L()
    _ran("wgemm", lambda: run_wgrad(True, N, 512, 256, 2, 2, 3, 1, L.X_BN_ACT, L.X_BN_DY))


# The all-taps kernel (32 x 32 tiles, layers with fewer than 64 channels on one side) has a pixel
# tail of its own.  In the shipped models those layers are the full-resolution ones, whose pixel
# count is a multiple of 256 at every batch, so only a thin layer on a small map reaches it (a
# hidden_dims list may put one there): 4N = 28 and 76 pixels.
THIN = [(False, 32, 32, 4, 2, 3, 1), (True, 32, 32, 2, 2, 3, 1)]


@pytest.mark.parametrize("N", [7, 19])
@pytest.mark.parametrize("shape", THIN)
def test_wgemm_taps_pixel_tail(shape, N):
    L = _L()
    tr, *rest = shape
    _ran("wgemm_taps_kernel", lambda: run_wgrad(tr, N, *rest, L.X_BN_ACT, L.X_BN_DY))


def test_cgemm_fwd_table_built_in_kernel():
    """Forward conv with BN_ACT from the raw statistics (no table): tab_build + running stats."""
    _cgemm_fwd_table_built_in_kernel(1)


def test_cgemm_fwd_table_built_from_replicated_stats():
    """The same from 4 replicas of the statistics (the plans' count at 64 channels)."""
    _cgemm_fwd_table_built_in_kernel(4)


def _cgemm_fwd_table_built_in_kernel(reps):
    L = _L()
    g = torch.Generator().manual_seed(9)
    N, cin, cout, hw = 8, 64, 128, 16
    y = bf(torch.randn(N, cin, hw, hw, generator=g) * 0.9 + 0.4)
    bn = BN(y, g, shift=torch.randn(cin, generator=g) * 0.05, reps=reps)
    w = bf(torch.randn(cout, cin, 3, 3, generator=g) * 0.1)
    ref = F.conv2d(bn.act().double(), w.double(), None, stride=2, padding=1)
    out = torch.empty(N, hw // 2, hw // 2, cout, device="cuda", dtype=torch.bfloat16)
    rm = torch.zeros(cin, device="cuda"); rv = torch.ones(cin, device="cuda")
    xf = bn.xf(L, L.X_BN_ACT)
    xf.running_mean, xf.running_var = rm.data_ptr(), rv.data_ptr()
    yd = nhwc(y)
    wd = w.permute(0, 2, 3, 1).contiguous().to("cuda", torch.bfloat16)
    a = L.ConvArgs(dtype=L.BF16, n=N, h=hw, w=hw, c=cin, k=cout, p=hw // 2, q=hw // 2, r=3, stride=2, pad=1)
    a.x = yd.data_ptr(); a.x_xf = xf; a.wt = wd.data_ptr(); a.y = out.data_ptr()
    L.call("vae_conv2d_fwd", ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert relmax(nchw(out), ref) < OUT_TOL
    mean = y.double().mean((0, 2, 3))
    var_u = y.double().var((0, 2, 3), unbiased=True)
    assert relmax(rm.cpu(), 0.1 * mean) < 1e-4
    assert relmax(rv.cpu() - 0.9, 0.1 * var_u) < 1e-4


# the VanillaVAE backward's nine weight gradients (B = 16): convT decoder, conv encoder, padded RGB
BATCH = [(True, 16, 64, 32, 16, 2, 3, 1), (True, 16, 128, 64, 8, 2, 3, 1), (True, 16, 256, 128, 4, 2, 3, 1),
         (True, 16, 512, 256, 2, 2, 3, 1), (False, 16, 256, 512, 4, 2, 3, 1), (False, 16, 128, 256, 8, 2, 3, 1),
         (False, 16, 64, 128, 16, 2, 3, 1), (False, 16, 32, 64, 32, 2, 3, 1), (False, 16, 8, 32, 64, 2, 3, 1)]


def run_wgrad_batch(N, fp32=False, layers=None):
    L = _L()
    ws = []
    for seed, (tr, _, cin, cout, hw, s_, R, pad) in enumerate(layers or BATCH):
        xk = L.X_BN_ACT if (tr and cin != 512) or (not tr and cin != 8) else L.X_NONE
        ws.append(prep_wgrad(tr, N, cin, cout, hw, s_, R, pad, xk, L.X_BN_DY, seed=10 + seed, fp32=fp32))
    n = len(ws)
    kinds = (ctypes.c_int32 * n)(*[L.LAYER_CONVT2D if w["fn"].startswith("vae_convT") else L.LAYER_CONV2D for w in ws])
    items = (ctypes.c_void_p * n)(*[ctypes.addressof(w["a"]) for w in ws])
    need = ctypes.c_size_t(0)
    L.call("vae_conv_bwd_filter_batch_workspace_size", n, kinds, items, ctypes.byref(need))
    wsb = torch.empty(max(16, need.value), dtype=torch.uint8, device="cuda")
    results = []
    for rep in range(2):
        for w in ws:
            for t in ("dw", "db", "dgo", "dbo"):
                w[t].zero_()
        L.call("vae_conv_bwd_filter_batch", n, kinds, items, wsb.data_ptr(), wsb.numel(),
               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        results.append([w["dw"].clone() for w in ws] + [w["db"].clone() for w in ws])
        if rep == 0:
            for w in ws:
                check_wgrad(w)
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_wgrad_batch_matches_reference_and_is_deterministic():
    """vae_conv_bwd_filter_batch (one XCD-partitioned grid, K-slice partials in slabs reduced in slice
    order): every layer's dW / bias / BN affine gradients against fp64, and two runs bit-identical."""
    run_wgrad_batch(16)


@pytest.mark.parametrize("N", [7, 19])
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_wgrad_batch_last_batch(N, mode):
    """The same nine layers at a partial last batch: the deep layers have 4N = 28 / 76 pixels, less
    than one 64-pixel K-step of the grouped kernel (wg3_kernel) / one step and a 12-pixel tail, and
    every layer's last K slice is ragged.  bf16: the grouped launch; fp32: the parity mode's calls
    with their partial sums added in a fixed order.  Reference, bars and the bit-identical rerun as above."""
    from gpu_util import launched
    log = launched(lambda: run_wgrad_batch(N, fp32=mode == "fp32"))
    if mode == "bf16":
        assert "wg3_kernel" in log and "wg3_reduce" in log, log
    else:       # the fp32 items run one by one on the VALU GEMM, K-split partials summed by its finalize
        assert "igemm_kernel<float" in log and "igemm_finalize<float" in log and "wg3_kernel" not in log, log


@pytest.mark.parametrize("N", [7, 19])
def test_wgrad_batch_thin_layers_pixel_tail(N):
    """The grouped launch's all-taps body (THIN above) with 28 / 76 pixels, beside one per-tap layer."""
    from gpu_util import launched
    layers = [(tr, N, *rest) for tr, *rest in THIN] + [(False, N, 256, 512, 4, 2, 3, 1)]
    log = launched(lambda: run_wgrad_batch(N, layers=layers))
    assert "wg3_kernel" in log, log
