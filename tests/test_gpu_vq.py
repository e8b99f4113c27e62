"""VQ-VAE (models/vq_vae.py) on the MI355X kernels: one teacher-forced training step against the
reference's golden vectors (tests/golden/vq_b4.npz, made by the reference's own VQVAE) and the
CPU oracle, plus the VectorQuantizer and Tanh/SSE kernels on their own.

Index exactness: the codebook indices must equal the reference's bit for bit on every row whose
distance gap (second-best minus best, recorded by the reference) exceeds 1e-5 — below that the
fp32 summation order of z·E decides, and the survey measured ties and order flips at that scale
(SURVEY.md §8(c)).  The rest of the step is then checked against the oracle teacher-forced with
the GPU's indices: loss terms within 1e-4 relative (north_star), reconstructions, per-image
MSE, every parameter gradient (norm within 1e-3), and the Adam update."""
import numpy as np
import pytest
import torch

from golden_util import case_inputs, load_case, summary

pytestmark = pytest.mark.gpu

GAP_EXACT = 1e-5


def _step(meta, dtype=torch.float32, batch=None, x=None):
    from vae_amd import _lib as L
    from vae_amd.engine import FusedAdam
    from vae_amd.vq import VQNet, VQStepPlan
    sd, x0, _ = case_inputs(meta)
    x = x0 if x is None else x
    kw = meta["ctor"]
    net = VQNet(embedding_dim=kw["embedding_dim"], num_embeddings=kw["num_embeddings"], dtype=dtype, device="cuda")
    net.load_reference_state_dict(sd)
    plan = VQStepPlan(net, x.shape[0], beta=kw["beta"])
    opt = FusedAdam(net, lr=meta["lr"])
    plan.x.copy_(x)
    st = L.stream_ptr()
    # step_begin zeroes the gradient region and advances the optimizer's step counter
    L.call("vae_step_begin", plan.zero.data_ptr(), plan.zero.numel() * 4, opt.step.data_ptr(), st)
    plan.forward(st)
    plan.backward(st)
    torch.cuda.synchronize()
    return sd, x, net, plan, opt


def test_vq_step_matches_reference():
    from oracle import vae_oracle as O
    meta, ref = load_case("vq_b4")
    sd, x, net, plan, opt = _step(meta)
    idx = plan.indices.cpu()
    want = torch.from_numpy(ref["indices"])
    gap = torch.from_numpy(ref["gap"])
    clear = gap > GAP_EXACT
    assert torch.equal(idx[clear], want[clear]), int((idx[clear] != want[clear]).sum())
    n_tie_flips = int((idx != want).sum())
    if n_tie_flips == 0:
        for k in ("loss", "Reconstruction_Loss", "VQ_Loss"):
            v = meta["loss"][k]
            assert abs(plan.loss_dict()[k] - v) <= 1e-4 * abs(v), (k, plan.loss_dict()[k], v)
    # teacher-forced oracle on the GPU's codes
    o = O.train_step("VQVAE", sd, x, M_N=0.0, lr=meta["lr"], vq_beta=meta["ctor"]["beta"], vq_indices=idx)
    got = plan.loss_dict()
    for k in ("loss", "Reconstruction_Loss", "VQ_Loss"):
        assert abs(got[k] - o["loss"][k]) <= 1e-4 * abs(o["loss"][k]), (k, got[k], o["loss"][k])
    np.testing.assert_allclose(plan.recon.cpu().numpy(), o["recon"].numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(plan.per_img.cpu().numpy(), o["per_img_mse"].numpy(), rtol=1e-4)
    grads = {k: v.cpu() for k, v in net.layout.export_reference(plan.grads).items()}
    assert set(grads) == set(o["grads"])
    for name, gr in o["grads"].items():
        g = grads[name]
        err = float((g - gr).norm() / gr.norm().clamp_min(1e-30))
        assert err < 1e-3, (name, err)
    # against the golden gradient summaries too when no near-tie row flipped
    if n_tie_flips == 0:
        for name in meta["param_names"]:
            st, rs = summary(grads[name]), ref[f"grad_stats/{name}"]
            assert abs(st[1] - rs[1]) <= 1e-3 * rs[1], (name, st, rs)
    # Adam from zero state: lr * g / (|g| + eps) on our gradients
    before = {k: v.cpu().double() for k, v in net.reference_state_dict().items()}
    opt.apply(plan.grads)
    torch.cuda.synchronize()
    after = {k: v.cpu().double() for k, v in net.reference_state_dict().items()}
    lr = meta["lr"]
    for name, g in grads.items():
        g = g.double()
        np.testing.assert_allclose(after[name].numpy(), (before[name] - lr * g / (g.abs() + 1e-8)).numpy(),
                                   rtol=0, atol=1e-6 * lr + 1e-7, err_msg=name)


def test_vq_step_bf16_close():
    """bf16 throughput mode at B=8: the indices equal the fp64 argmin over the step's own bf16
    latents on every clear row; loss terms within 2e-2 of the teacher-forced oracle."""
    from gpu_util import check_vq_indices
    from oracle import vae_oracle as O
    meta, _ = load_case("vq_b4")
    x = torch.rand(8, 3, 64, 64, generator=torch.Generator().manual_seed(7))
    sd, x, net, plan, opt = _step(meta, torch.bfloat16, x=x)
    check_vq_indices(plan.latpre, sd["vq_layer.embedding.weight"], plan.indices, "VQ B=8 bf16")
    o = O.train_step("VQVAE", sd, x, M_N=0.0, lr=meta["lr"], vq_beta=meta["ctor"]["beta"],
                     vq_indices=plan.indices.cpu(), do_adam=False)
    got = plan.loss_dict()
    for k, tol in (("loss", 2e-2), ("Reconstruction_Loss", 2e-2), ("VQ_Loss", 5e-2)):
        assert abs(got[k] - o["loss"][k]) <= tol * abs(o["loss"][k]), (k, got[k], o["loss"][k])


@pytest.mark.parametrize("rows,codes,dim", [(1000, 512, 64), (333, 100, 32), (64, 7, 16)])
def test_vq_kernel_vs_torch(rows, codes, dim):
    """vae_vq_fwd / vae_vq_bwd against the reference's formulas in torch fp32 (CPU)."""
    from vae_amd import _lib as L
    g = torch.Generator().manual_seed(rows + codes)
    pre = torch.randn(rows, dim, generator=g)
    E = (torch.rand(codes, dim, generator=g) * 2 - 1) * 0.5
    E[codes // 2] = E[0]                                   # exact duplicate code: tie -> first index
    dq = torch.randn(rows, dim, generator=g) * 1e-3
    beta = 0.25
    lat_d, E_d, dq_d = pre.cuda(), E.cuda(), dq.cuda()
    idx = torch.zeros(rows, dtype=torch.int64, device="cuda")
    q = torch.empty(rows, dim, device="cuda")
    sse = torch.zeros(1, device="cuda")
    dlat = torch.empty(rows, dim, device="cuda")
    dE = torch.zeros(codes, dim, device="cuda")
    a = L.VqArgs(dtype=L.F32, rows=rows, dim=dim, codes=codes, beta=beta)
    a.lat, a.lat_xf = lat_d.data_ptr(), L.Xform(kind=L.X_ACT, channels=1, slope=0.01)
    a.codebook, a.indices, a.q, a.sse = E_d.data_ptr(), idx.data_ptr(), q.data_ptr(), sse.data_ptr()
    a.dq, a.dlat, a.dcodebook = dq_d.data_ptr(), dlat.data_ptr(), dE.data_ptr()
    st = L.stream_ptr()
    L.call("vae_vq_fwd", a, st)
    L.call("vae_vq_bwd", a, st)
    torch.cuda.synchronize()
    # reference formulas (vq_vae.py:24-55) with autograd
    z = torch.nn.functional.leaky_relu(pre, 0.01).requires_grad_(True)
    Ew = E.clone().requires_grad_(True)
    dist = torch.sum(z ** 2, dim=1, keepdim=True) + torch.sum(Ew ** 2, dim=1) - 2 * torch.matmul(z, Ew.t())
    want = torch.argmin(dist, dim=1)
    top2 = torch.topk(dist.detach(), 2, dim=1, largest=False).values
    clear = (top2[:, 1] - top2[:, 0]) > GAP_EXACT
    got = idx.cpu()
    assert torch.equal(got[clear], want[clear])
    assert int((got == codes // 2).sum()) == 0          # the duplicate of code 0 never wins the tie
    onehot = torch.zeros(rows, codes).scatter_(1, got.view(-1, 1), 1)
    qq = onehot @ Ew
    vq_loss = torch.nn.functional.mse_loss(qq.detach(), z) * beta + torch.nn.functional.mse_loss(qq, z.detach())
    st_q = z + (qq - z).detach()
    (vq_loss + (st_q * dq).sum()).backward()
    pre_g = z.grad * torch.where(pre > 0, 1.0, 0.01)
    np.testing.assert_allclose(q.cpu().numpy(), qq.detach().numpy(), rtol=0, atol=0)
    assert abs(float(sse) * (1 + beta) / (rows * dim) - float(vq_loss)) <= 1e-5 * float(vq_loss)
    np.testing.assert_allclose(dlat.cpu().numpy(), pre_g.numpy(), rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(dE.cpu().numpy(), Ew.grad.numpy(), rtol=1e-4, atol=1e-9)


def _vq_call(dtype, pre, E, act, dq=None, beta=0.25, s=None, dE0=None):
    """vae_vq_fwd (and vae_vq_bwd when dq is given) through the C ABI with VQStepPlan's operand
    types: lat / q / dq / dlat in `dtype`, codebook / dcodebook / sse fp32, indices int64.
    Returns the outputs on the CPU and the launch log."""
    from gpu_util import launched
    from vae_amd import _lib as L
    rows, dim = pre.shape
    codes = E.shape[0]
    lat_d, E_d = pre.to("cuda", dtype), E.cuda()
    idx = torch.full((rows,), -1, dtype=torch.int64, device="cuda")
    q = torch.empty(rows, dim, device="cuda", dtype=dtype)
    sse = torch.zeros(1, device="cuda")
    a = L.VqArgs(dtype=L.dtype_code(dtype), rows=rows, dim=dim, codes=codes, beta=beta)
    a.lat = lat_d.data_ptr()
    a.lat_xf = L.Xform(kind=L.X_ACT, channels=1, slope=0.01) if act else L.Xform(kind=L.X_NONE)
    a.codebook, a.indices, a.q, a.sse = E_d.data_ptr(), idx.data_ptr(), q.data_ptr(), sse.data_ptr()
    st = L.stream_ptr()
    out, keep = {}, []
    if dq is not None:
        dq_d = dq.to("cuda", dtype)
        dlat = torch.empty(rows, dim, device="cuda", dtype=dtype)
        dE = torch.zeros(codes, dim, device="cuda") if dE0 is None else dE0.clone().cuda()
        a.dq, a.dlat, a.dcodebook = dq_d.data_ptr(), dlat.data_ptr(), dE.data_ptr()
        if s is not None:
            keep.append(torch.full((1,), s, device="cuda"))
            a.loss_grad = keep[0].data_ptr()

    def run():
        L.call("vae_vq_fwd", a, st)
        if dq is not None:
            L.call("vae_vq_bwd", a, st)
    out["log"] = launched(run)
    torch.cuda.synchronize()
    if dq is not None:
        out.update(dlat=dlat.float().cpu(), dE=dE.cpu())
    out.update(idx=idx.cpu(), q=q.float().cpu(), sse=float(sse))
    return out


# rows, codes, dim, lat_xf ACT (else NONE), loss_grad scalar (else NULL), dcodebook starts nonzero
VQ_OP_CASES = [
    (1000, 512, 64, True, None, False),    # the step's shape and arguments: four full 128-code chunks
    (333, 200, 32, True, 0.37, False),     # a full chunk, then 72 codes: ragged last 16-code block
    (257, 129, 64, False, None, True),     # second chunk of one code; 4 full workgroups + 1 row
    (130, 1100, 16, False, 0.37, True),    # nine chunks; codes > 1024: bwd on the LM=false kernel
    (64, 7, 16, True, None, False),        # fewer codes than one 16-lane block
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,codes,dim,act,s,acc", VQ_OP_CASES)
def test_vq_kernel_vs_fp64(rows, codes, dim, act, s, acc, dtype):
    """vae_vq_fwd / vae_vq_bwd in fp32 and in bf16 (vq_fwd_kernel<__bf16, D, 1>, vq_bwd_kernel<__bf16, LM>)
    against the reference's formulas (vq_vae.py:24-55) in fp64, evaluated on the values the kernel
    reads (the bf16-rounded latents and dq in bf16 mode).

    Branches reached (csrc/vae_vq.hip): a partial last LDS chunk after a full one (codes 200, 129,
    1100); a last 16-code block with idle lanes (200, 129, 1100, 7); the last workgroup with one row
    (257); vq_bwd_kernel<T, false>, direct global atomics (codes 1100 > 1024); lat_xf NONE (two
    cases) and ACT; loss_grad != NULL (two cases, s = 0.37: it scales the commitment and embedding
    terms, not dq, so the reference loss is s·vq_loss + (st_q·dq).sum()); dcodebook accumulated
    onto a nonzero start (two cases, one per bwd kernel).

    Indices are exact on every clear row (gpu_util.vq_argmin_clear: gap above twice the worst-case
    fp32 rounding of the distance formula), and at least 95 % of the rows must be clear — measured
    on the CPU for these seeds: 100 % in every case but 257 x 129 x 64 in bf16 (one row short, 99.6 %)."""
    from gpu_util import vq_argmin_clear
    beta = 0.25
    g = torch.Generator().manual_seed(rows + codes)
    pre = torch.randn(rows, dim, generator=g).to(dtype).float()
    E = (torch.rand(codes, dim, generator=g) * 2 - 1) * 0.5
    dq = (torch.randn(rows, dim, generator=g) * 1e-3).to(dtype).float()
    # the nonzero start has the gradient's own scale 2 / (rows·dim), so that the fp32 rounding of
    # start + increment (2⁻²⁴ of it) stays far below the increment's 1e-9 absolute bar
    dE0 = torch.randn(codes, dim, generator=g) * (2.0 / (rows * dim)) if acc else torch.zeros(codes, dim)
    out = _vq_call(dtype, pre, E, act, dq=dq, beta=beta, s=s, dE0=dE0)
    got = out["idx"]
    # the instantiations this case is here for, <element type, dim, 1> and <element type, LM>, by
    # their mangled names (f = float, DF16b = __bf16, which not every demangler knows)
    ty = "f" if dtype == torch.float32 else "DF16b"
    assert f"vq_fwd_kernelI{ty}Li{dim}ELi1EE" in out["log"], out["log"]
    assert f"vq_bwd_kernelI{ty}Lb{int(codes <= 1024)}EE" in out["log"], out["log"]
    # the kernel's own fp32 activation of the stored latent, then everything in fp64
    slope = float(torch.tensor(0.01, dtype=torch.float32))
    z = (torch.nn.functional.leaky_relu(pre, 0.01) if act else pre).double().requires_grad_(True)
    Ew = E.double().requires_grad_(True)
    want, clear = vq_argmin_clear(z.detach(), E)
    share = float(clear.double().mean())
    assert int(got.min()) >= 0 and int(got.max()) < codes, (int(got.min()), int(got.max()))
    mism = int((got[clear] != want[clear]).sum())
    assert share >= 0.95, share
    assert mism == 0, mism
    qq = Ew[got]
    mse = torch.nn.functional.mse_loss
    vq_loss = mse(qq.detach(), z) * beta + mse(qq, z.detach())
    st_q = z + (qq - z).detach()
    sv = 1.0 if s is None else float(torch.tensor(s, dtype=torch.float32))
    (sv * vq_loss + (st_q * dq.double()).sum()).backward()
    pre_g = z.grad * torch.where(pre > 0, 1.0, slope).double() if act else z.grad
    assert torch.equal(out["q"], E[got].to(dtype).float())
    e_sse = abs(out["sse"] * (1 + beta) / (rows * dim) - float(vq_loss)) / float(vq_loss)
    d_lat = (out["dlat"].double() - pre_g).abs()
    inc = out["dE"].double() - dE0.double()
    d_E = (inc - Ew.grad).abs()
    print(f"vq {rows}x{codes}x{dim} {'bf16' if dtype == torch.bfloat16 else 'fp32'}: clear {100 * share:.2f} %, "
          f"sse rel {e_sse:.2e}, dlat max rel {float((d_lat / pre_g.abs().clamp_min(1e-6)).max()):.2e}, "
          f"dcodebook max err / max {float(d_E.max() / Ew.grad.abs().max()):.2e}")
    assert e_sse <= 1e-5, e_sse
    if dtype == torch.float32:
        np.testing.assert_allclose(out["dlat"].numpy(), pre_g.numpy(), rtol=1e-5, atol=1e-9)
    else:
        # one bf16 rounding of an fp32 value.  bf16 keeps 8 significant bits, so round-to-nearest is
        # off by at most 2⁻⁸ / (1 + 2⁻⁸) of the value (reached just above a power of two: 3.89e-3
        # measured in every case); the fp32 value's own error, 2e-6 here, fits in the 1.5e-5 left
        assert bool((d_lat <= 2.0 ** -8 * pre_g.abs() + 1e-9).all()), float((d_lat - 2.0 ** -8 * pre_g.abs()).max())
    np.testing.assert_allclose(inc.numpy(), Ew.grad.numpy(), rtol=1e-4, atol=1e-9)
    unpicked = torch.bincount(got, minlength=codes) == 0
    assert torch.equal(out["dE"][unpicked], dE0[unpicked])      # codes no row picked: untouched, bit for bit


# duplicate code -> the base code it copies bit for bit
VQ_TIE_DUPS = {1: 0, 21: 5, 140: 9, 33: 2, 290: 2}


def _vq_tie_case(dtype):
    """(pre, E, planted rows, their expected index) of the forced-tie test: codes 300, dim 64,
    rows 128 (two workgroups), bf16-representable codebook values so that a latent can equal a
    code bit for bit in both dtypes."""
    g = torch.Generator().manual_seed(300)
    E = ((torch.rand(300, 64, generator=g) * 2 - 1) * 0.5).bfloat16().float()
    for dup, base in VQ_TIE_DUPS.items():
        E[dup] = E[base]
    pre = torch.randn(128, 64, generator=g).to(dtype).float()
    # every third row: rows 0, 3, ..., 126 sit at 43 different positions of the 64-row tile (all
    # four waves, all four accumulator rows of a lane), cycling through the four base codes
    planted = torch.arange(0, 128, 3)
    expect = torch.tensor([0, 5, 9, 2])[(planted // 3) % 4]
    pre[planted] = E[expect]
    return pre, E, planted, expect


def _check_vq_ties(got, planted, expect):
    """The planted rows got the smallest index of their tied set; a duplicate ties bit for bit
    with its base code on EVERY row, so under first-minimum it wins nowhere."""
    assert torch.equal(got[planted], expect), (got[planted].tolist(), expect.tolist())
    dups = torch.tensor(sorted(VQ_TIE_DUPS))
    assert not bool(torch.isin(got, dups).any()), got[torch.isin(got, dups)].tolist()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_vq_first_minimum_on_forced_ties(dtype):
    """torch.argmin's first-minimum tie-break at each level of vq_fwd_kernel, forced: a third of the
    rows EQUAL a code that has exact duplicates, so the duplicates share the minimum distance bit
    for bit (same data, same fma order) and only the tie-break decides.
      E[1] = E[0]      neighbouring lane of the same 16-code block: the (distance, index) shuffle combine
      E[21] = E[5]     same lane (code % 16), next block: strict < in the lane's ascending scan
      E[140] = E[9]    next 128-code LDS chunk, another lane: lane 9's best, carried in registers
                       over the two later chunks, against lane 12's equal one in the combine
      E[33] = E[290] = E[2]   290 in lane 2 two chunks later (strict < against the carried best) and
                       33 in lane 1 (combine): two levels at once
    codes 300 also ends in a partial chunk (44 codes); lat_xf NONE.  A stand-in that breaks ties
    toward the LAST index fails _check_vq_ties on every planted row (checked on the CPU)."""
    from gpu_util import vq_argmin_clear
    pre, E, planted, expect = _vq_tie_case(dtype)
    out = _vq_call(dtype, pre, E, act=False)
    got = out["idx"]
    assert int(got.min()) >= 0 and int(got.max()) < 300
    _check_vq_ties(got, planted, expect)
    assert torch.equal(out["q"][planted], E[expect])            # bf16-representable: exact in both dtypes
    # the random rows: exact wherever the fp64 argmin is clear (a row nearest to a duplicated code
    # has gap 0 and is not)
    want, clear = vq_argmin_clear(pre, E)
    assert torch.equal(got[clear], want[clear])


@pytest.mark.parametrize("dtype,ld", [(torch.float32, 0), (torch.bfloat16, 0), (torch.float32, 8), (torch.bfloat16, 8)])
def test_recon_kernel(dtype, ld):
    """vae_recon_fwd / vae_recon_bwd: tanh, per-image SSE, d/dy of mse(tanh(y), x); ld 8 = the
    packed RGB ends (3 channels in rows of 8: padding ignored on load, written as zeros in dy)."""
    from vae_amd import _lib as L
    g = torch.Generator().manual_seed(3)
    n, hw = 3, 32
    row = ld if ld else 3
    y_full = torch.randn(n, hw, hw, row, generator=g).to(dtype)
    y = y_full[..., :3]
    x = torch.rand(n, 3, hw, hw, generator=g)
    y_d, x_d = y_full.cuda(), x.cuda()
    recon = torch.empty(n, 3, hw, hw, device="cuda")
    sse = torch.zeros(n, device="cuda")
    dy_full = torch.full((n, hw, hw, row), 7.0, dtype=dtype, device="cuda")
    dy = dy_full[..., :3]
    a = L.ReconArgs(dtype=L.dtype_code(dtype), n=n, h=hw, w=hw, c=3, ld=ld, grad_scale=1.0 / x.numel())
    a.y, a.target, a.recon, a.sse, a.dy = y_d.data_ptr(), x_d.data_ptr(), recon.data_ptr(), sse.data_ptr(), dy_full.data_ptr()
    L.call("vae_recon_fwd", a, L.stream_ptr())
    torch.cuda.synchronize()
    if ld:
        assert float(dy_full[..., 3:].float().abs().max()) == 0.0
    yr = y.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    r = torch.tanh(yr)
    loss = torch.nn.functional.mse_loss(r, x)
    loss.backward()
    tolr = 1e-6 if dtype == torch.float32 else 1e-2
    np.testing.assert_allclose(recon.cpu().numpy(), r.detach().numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(sse.cpu().numpy(), ((r.detach() - x) ** 2).sum(dim=(1, 2, 3)).numpy(), rtol=1e-5)
    want_dy = yr.grad.permute(0, 2, 3, 1)
    np.testing.assert_allclose(dy.float().cpu().numpy(), want_dy.numpy(), rtol=tolr, atol=tolr * float(want_dy.abs().max()))
    # bwd from a caller-supplied dL/drecon
    gr = torch.randn(n, 3, hw, hw, generator=g)
    gr_d = gr.cuda()
    b = L.ReconArgs(dtype=L.dtype_code(dtype), n=n, h=hw, w=hw, c=3, ld=ld)
    b.target, b.recon, b.dy, b.grad_recon = x_d.data_ptr(), recon.data_ptr(), dy_full.data_ptr(), gr_d.data_ptr()
    L.call("vae_recon_bwd", b, L.stream_ptr())
    torch.cuda.synchronize()
    want = (gr * (1 - r.detach() ** 2)).permute(0, 2, 3, 1)
    np.testing.assert_allclose(dy.float().cpu().numpy(), want.numpy(), rtol=tolr, atol=tolr * float(want.abs().max()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("r,pad", [(3, 1), (1, 0)])
def test_conv_stride1_bwd_data_residual_act(dtype, r, pad):
    """conv2d_bwd_data at stride 1 (the ResidualLayer convs, vq_vae.py:62-66): dx = W^T * dy + skip,
    times lrelu'(x_pre) — against torch autograd in fp32 (bf16 runs the flipped-weight conv path)."""
    from gpu_util import give_workspace, nhwc, to_nchw
    from vae_amd import _lib as L
    g = torch.Generator().manual_seed(11 + r)
    n, hw, c, k = 2, 8, 32, 64
    x_pre = torch.randn(n, c, hw, hw, generator=g)
    w = torch.randn(k, c, r, r, generator=g) * 0.1
    dy = torch.randn(n, k, hw, hw, generator=g)
    skip = torch.randn(n, c, hw, hw, generator=g)
    xa = torch.nn.functional.leaky_relu(x_pre, 0.01).requires_grad_(True)
    y = torch.nn.functional.conv2d(xa, w, None, padding=pad)
    (y * dy).sum().backward()
    want = (xa.grad + skip) * torch.where(x_pre > 0, 1.0, 0.01)
    dev = dict(dtype=dtype)
    wn = w.permute(0, 2, 3, 1).contiguous().to(device="cuda", **dev)
    dy_d, skip_d, xp_d = nhwc(dy, dtype), nhwc(skip, dtype), nhwc(x_pre, dtype)
    dx = torch.empty_like(xp_d)
    a = L.ConvArgs(dtype=L.dtype_code(dtype), n=n, h=hw, w=hw, c=c, k=k, p=hw, q=hw, r=r, stride=1, pad=pad)
    a.dy, a.wt, a.dx, a.residual = dy_d.data_ptr(), wn.data_ptr(), dx.data_ptr(), skip_d.data_ptr()
    a.dx_epi = L.Xform(kind=L.X_ACT, channels=c, slope=0.01)
    a.dx_epi.aux = xp_d.data_ptr()
    ws = give_workspace(a, "vae_conv2d_bwd_data")
    L.call("vae_conv2d_bwd_data", a, L.stream_ptr())
    torch.cuda.synchronize()
    got = to_nchw(dx)
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    err = float((got - want).abs().max() / want.abs().max())
    assert err < tol, err


def test_vq_bf16_gradients_close_to_oracle():
    """bf16 VQ-VAE step (padded 8-channel image and output ConvT) against the teacher-forced fp32
    oracle: gradients of the padded layers and the codebook within 5e-2 relative norm."""
    from oracle import vae_oracle as O
    meta, _ = load_case("vq_b4")
    sd, x, net, plan, opt = _step(meta, torch.bfloat16)
    o = O.train_step("VQVAE", sd, x, M_N=0.0, lr=meta["lr"], vq_beta=meta["ctor"]["beta"],
                     vq_indices=plan.indices.cpu(), do_adam=False)
    grads = {k: v.cpu() for k, v in net.layout.export_reference(plan.grads).items()}
    for name in ("encoder.0.0.weight", "encoder.0.0.bias", "decoder.9.0.weight", "decoder.9.0.bias",
                 "vq_layer.embedding.weight", "decoder.8.0.weight"):
        err = float((grads[name] - o["grads"][name]).norm() / o["grads"][name].norm())
        assert err < 5e-2, (name, err)
