"""vae_latent_* (the bf16 bottleneck: fc_mu|fc_var, reparameterize, decoder_input and their
backward; vaehip.h) and vae_step_begin_ex against PyTorch fp32 on the same bf16-rounded operands.

Reference ops: models/vanilla_vae.py:36-37 / :89-90 (fc_mu, fc_var), :107-117 (reparameterize),
:43 / :101 (decoder_input), with the encoder's last BatchNorm2d + LeakyReLU (:30-31) applied to the
stored pre-BN map on load.  The kernels accumulate fp32 in a different order and split K over
workgroups with fp32 atomics, so the bars are relative to each tensor's max: 2e-3 for fp32 outputs
of bf16 operands, one bf16 ulp (2^-8) plus that for bf16 outputs.
"""
import pytest
import torch
import torch.nn.functional as Fn

from gpu_util import BNState, rel
from vae_amd import _lib as L

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _bf(t):
    return t.to(BF).float()


def _setup(B, S, D=128, C=512, N2=2048, seed=0, reps=2):
    g = torch.Generator().manual_seed(seed)
    K1 = 4 * C
    y = torch.randn(B, C, 2, 2, generator=g) * 1.5 + 0.3                # pre-BN map, NCHW
    bn = BNState(_bf(y), shift=torch.randn(C, generator=g) * 0.1, seed=seed + 1, dtype=BF)
    # the producer's sums split over `reps` replicas (the kernels reduce them)
    rs = torch.stack([bn.sum * 0.25, bn.sum * 0.75]) if reps == 2 else bn.sum[None]
    rq = torch.stack([bn.sumsq * 0.5, bn.sumsq * 0.5]) if reps == 2 else bn.sumsq[None]
    dev = dict(device="cuda")
    T = dict(
        y=bn,
        rsum=rs.contiguous().cuda(), rsq=rq.contiguous().cuda(),
        w1=_bf(torch.randn(2 * D, K1, generator=g) * 0.02), b1=torch.randn(2 * D, generator=g) * 0.1,
        w2=_bf(torch.randn(N2, D, generator=g) * 0.05), b2=torch.randn(N2, generator=g) * 0.1,
        eps=torch.randn(B * S, D, generator=g),
        dh=_bf(torch.randn(B * S, N2, generator=g) * 0.01),
        kl=torch.randn(B * S, generator=g) * 0.01,
    )
    T["x"] = bn.y_dev.reshape(B, K1)                                    # NHWC flatten = native In'
    T["mulv"] = torch.zeros(B, 2 * D, **dev)
    T["z"] = torch.zeros(B * S, D, dtype=BF, **dev)
    T["h"] = torch.zeros(B * S, N2, dtype=BF, **dev)
    T["dmulv"] = torch.zeros(B, 2 * D, **dev)
    T["dw1"] = torch.zeros(2 * D, K1, **dev)
    T["db1"] = torch.zeros(2 * D, **dev)
    T["dw2"] = torch.zeros(N2, D, **dev)
    T["db2"] = torch.zeros(N2, **dev)
    T["dx"] = torch.zeros(B, K1, dtype=BF, **dev)
    T["dsum"] = torch.zeros(2, reps, C, **dev)
    T["run_m"] = torch.zeros(C, **dev)
    T["run_v"] = torch.ones(C, **dev)
    for k in ("w1", "w2"):
        T[k + "_d"] = T[k].to(BF).cuda()
    for k in ("b1", "b2", "eps", "kl"):
        T[k + "_d"] = T[k].cuda()
    T["dh_d"] = T["dh"].to(BF).cuda()

    def xf(aux=False):
        x = bn.xf(L.X_BN_ACT, aux=T["x"] if aux else None)
        x.sum, x.sumsq = T["rsum"].data_ptr(), T["rsq"].data_ptr()
        x.reps, x.rstride = reps, C
        if not aux:
            x.running_mean, x.running_var = T["run_m"].data_ptr(), T["run_v"].data_ptr()
        return x

    a = L.LatentArgs(dtype=L.BF16, batch=B, samples=S, latent=D, in_features=K1, out_features=N2)
    a.x, a.x_xf = T["x"].data_ptr(), xf()
    a.w1, a.b1, a.mulv = T["w1_d"].data_ptr(), T["b1_d"].data_ptr(), T["mulv"].data_ptr()
    a.eps, a.z = T["eps_d"].data_ptr(), T["z"].data_ptr()
    a.w2, a.b2, a.h = T["w2_d"].data_ptr(), T["b2_d"].data_ptr(), T["h"].data_ptr()
    a.dh, a.kl_coef, a.dmulv = T["dh_d"].data_ptr(), T["kl_d"].data_ptr(), T["dmulv"].data_ptr()
    a.dw2, a.db2 = T["dw2"].data_ptr(), T["db2"].data_ptr()
    a.dx, a.dx_epi = T["dx"].data_ptr(), xf(aux=True)
    a.dx_dgamma, a.dx_dbeta = T["dsum"][0].data_ptr(), T["dsum"][1].data_ptr()
    a.sum_reps, a.sum_rstride = reps, C
    a.dw1, a.db1 = T["dw1"].data_ptr(), T["db1"].data_ptr()
    return a, T


def _ref(T, B, S, D, C):
    """fp32 PyTorch restatement of the four calls (NHWC flatten, bf16-rounded MFMA operands)."""
    bn = T["y"]
    K1 = 4 * C
    y = bn.y_nchw                                                      # bf16 values
    mean = bn.sum / bn.count + bn.shift
    var = (bn.sumsq / bn.count - (bn.sum / bn.count) ** 2).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    a_c = bn.gamma * invstd
    b_c = bn.beta - mean * a_c
    yn = y.permute(0, 2, 3, 1).reshape(B, K1)                          # NHWC flatten
    ch = torch.arange(K1) % C
    zbn = yn * a_c[ch] + b_c[ch]
    act = _bf(Fn.leaky_relu(zbn, 0.01))
    mulv = act @ T["w1"].t() + T["b1"]
    mu, lv = mulv[:, :D], mulv[:, D:]
    rows = torch.arange(B * S) // S
    z = _bf(T["eps"] * torch.exp(0.5 * lv[rows]) + mu[rows])
    h = z @ T["w2"].t() + T["b2"]
    # backward
    dz = T["dh"] @ T["w2"]
    c = T["kl"][:, None]
    dmu_r = dz + c * mu[rows]
    dlv_r = dz * T["eps"] * 0.5 * torch.exp(0.5 * lv[rows]) + c * 0.5 * (torch.exp(lv[rows]) - 1)
    dmulv = torch.zeros(B, 2 * D).index_add_(0, rows, torch.cat([dmu_r, dlv_r], 1))
    dw2 = T["dh"].t() @ z
    db2 = T["dh"].sum(0)
    dH = _bf(dmulv) @ T["w1"]
    g = torch.where(zbn > 0, dH, dH * 0.01)
    xhat = (yn - mean[ch]) * invstd[ch]
    sg = torch.zeros(C).index_add_(0, ch, g.sum(0))
    sgx = torch.zeros(C).index_add_(0, ch, (g * xhat).sum(0))
    dw1 = _bf(dmulv).t() @ act
    db1 = dmulv.sum(0)
    run_m = 0.1 * mean
    run_v = 0.9 + 0.1 * var * bn.count / (bn.count - 1)
    return dict(mulv=mulv, z=z, h=h, dmulv=dmulv, dw2=dw2, db2=db2, dx=g, sg=sg, sgx=sgx, dw1=dw1, db1=db1,
                run_m=run_m, run_v=run_v)


# (1, 1) .. (13, 5): the partial last batch of an epoch.  1, 7 and 3 x 5 = 15 rows are less than one
# 32- / 64-row tile and one 64-row K chunk of the dW2 / dW1 tiles, 19 rows a tile and a 64-row chunk
# with a tail, 13 x 5 = 65 rows one past a 64-row tile: the false branches of the kernels' row guards.
@pytest.mark.parametrize("B,S", [(64, 1), (32, 1), (64, 5), (1, 1), (7, 1), (19, 1), (3, 5), (13, 5)])
def test_latent_forward_backward_matches_torch(B, S):
    from gpu_util import launched
    D, C = 128, 512
    a, T = _setup(B, S, D=D, C=C)
    st = L.stream_ptr()

    def run():
        L.call("vae_latent_fc_fwd", a, st)
        L.call("vae_latent_dec_fwd", a, st)
        torch.cuda.synchronize()
        # the backward reads the reference's d[mu|logvar] seeds only through dh / kl_coef
        L.call("vae_latent_dec_bwd", a, st)
        L.call("vae_latent_fc_bwd", a, st)
        torch.cuda.synchronize()

    log = launched(run)
    for k in ("latent_fc_fwd_kernel", "latent_dec_fwd_kernel", "latent_dec_bwd_kernel", "latent_fc_bwd_kernel"):
        assert k in log, log
    R = _ref(T, B, S, D, C)
    got = T["dsum"].sum(1).cpu()                       # replicas summed: [Sg*xhat (dgamma), Sg (dbeta)]
    checks = [("mulv", T["mulv"], R["mulv"], 2e-3), ("z", T["z"].float(), R["z"], 1e-2),
              ("h", T["h"].float(), R["h"], 1.2e-2), ("run_m", T["run_m"], R["run_m"], 1e-4),
              ("run_v", T["run_v"], R["run_v"], 1e-4), ("dmulv", T["dmulv"], R["dmulv"], 2e-3),
              ("dw2", T["dw2"], R["dw2"], 2e-3), ("db2", T["db2"], R["db2"], 1e-4),
              ("dx", T["dx"].float(), R["dx"], 1.5e-2), ("sg", got[1], R["sg"], 1e-2), ("sgx", got[0], R["sgx"], 1e-2),
              ("dw1", T["dw1"], R["dw1"], 5e-3), ("db1", T["db1"], R["db1"], 1e-3)]
    errs = [(name, rel(g.cpu(), r), bar) for name, g, r, bar in checks]
    print(f"latent B={B} S={S}: " + ", ".join(f"{n} {e:.2e}/{b:g}" for n, e, b in errs))
    for name, e, bar in errs:
        assert e < bar, (name, e, bar)


def test_latent_rejects_unsupported_shapes():
    a, _ = _setup(8, 1)
    a.latent = 96
    with pytest.raises(L.VaeHipError):
        L.call("vae_latent_fc_fwd", a, L.stream_ptr())
    a.latent, a.dtype = 128, L.F32
    with pytest.raises(L.VaeHipError):
        L.call("vae_latent_dec_fwd", a, L.stream_ptr())


def test_step_begin_ex_matches_separate_calls():
    """vae_step_begin_ex == vae_step_begin + vae_nchw_to_nhwc_pad + vae_pad_channels x2."""
    g = torch.Generator().manual_seed(3)
    B, img = 5, 64
    x = torch.rand(B, 3, img, img, generator=g).cuda()
    zero = torch.randn(1001, generator=g).cuda()                        # 4004 bytes: a 4-byte tail
    step = torch.tensor([7], dtype=torch.int32).cuda()
    w = [torch.randn(r, 3, generator=g).to(BF).cuda() for r in (288, 512)]
    y = torch.full((B, img, img, 8), 9.0, dtype=BF).cuda()
    wd = [torch.full((t.shape[0], 8), 9.0, dtype=BF).cuda() for t in w]
    a = L.StepBeginArgs(zero=zero.data_ptr(), bytes=zero.numel() * 4, step=step.data_ptr(), dtype=L.BF16,
                        n=B, c=3, h=img, w=img, cp=8, x=x.data_ptr(), y=y.data_ptr(), npad=2)
    for i in range(2):
        a.pad[i] = L.PadDesc(rows=w[i].shape[0], c=3, cp=8, src=w[i].data_ptr(), dst=wd[i].data_ptr())
    L.call("vae_step_begin_ex", a, L.stream_ptr())
    torch.cuda.synchronize()
    assert int(step.item()) == 8
    assert float(zero.abs().max()) == 0.0
    want = torch.zeros(B, img, img, 8)
    want[..., :3] = x.cpu().permute(0, 2, 3, 1)
    assert torch.equal(y.float().cpu(), want.to(BF).float())
    for t, d in zip(w, wd):
        ref = torch.zeros(t.shape[0], 8, dtype=BF)
        ref[:, :3] = t.cpu()
        assert torch.equal(d.cpu(), ref)
