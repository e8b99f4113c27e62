"""vae_mmd_fwd / vae_mmd_reseed (csrc/vae_mmd.hip) against the reference's compute_mmd
(models/info_vae.py:150-229, restated in tests/infovae_ref.py) in fp64 torch with autograd.

Bars: mmd within 1e-4 relative of fp64 (the project's fp32 loss bar; the reference's own fp32 result
sits 3e-6..6e-6 (imq) and 5e-7 (rbf) from fp64 at B = 4 / 16 / 64), dz within 1e-4 relative norm of the
fp64 gradient.  Each case prints fp32 torch's own distance from fp64, so the margin is on record.
The mmd value is read the way a step reads it: vae_elbo_fwd (VAE_LOSS_INFO) adds the partials.

Shapes: B = 2 (one row pair), 4, 16 (one full tile), 24 (ragged tile), 48 and 64 (several tiles; 64 is
the config's batch), 144 (more than one column pass of both kernels' column tiles); D = 32, 128
(128-wide instantiation) and 256 (the 256-wide one)."""
import ctypes

import pytest
import torch

import infovae_ref as R

pytestmark = pytest.mark.gpu

KINDS = {"imq": 0, "rbf": 1}


def _inputs(B, D, seed=0):
    g = torch.Generator().manual_seed(1000 * B + D + seed)
    mulv = torch.cat([0.5 * torch.randn(B, D, generator=g), 0.3 * torch.randn(B, D, generator=g)], 1)
    eps = torch.randn(B, D, generator=g)
    prior = torch.randn(B, D, generator=g)
    return mulv, eps, prior


def run_mmd(mulv, eps, prior, kind, latent_var=2.0, grad_scale=1.0, dmulv=None, prior_gen=None):
    """One vae_mmd_fwd + the consumer's ordered sum.  Returns dict(mmd, dz, partials, prior, dmulv).
    prior_gen: (step tensor, seed) to draw the prior on the device."""
    from vae_amd import _lib as L
    B, D = eps.shape
    dev = "cuda"
    f = dict(dtype=torch.float32, device=dev)
    mulv_d, eps_d = mulv.to(**f).contiguous(), eps.to(**f).contiguous()
    prior_d = prior.to(**f).contiguous() if prior is not None else torch.zeros(B, D, **f)
    dz = torch.full((B, D), float("nan"), **f)
    a = L.MmdArgs(kind=KINDS[kind], batch=B, latent=D, latent_var=latent_var, grad_scale=grad_scale)
    a.mulv, a.eps, a.prior, a.dz = mulv_d.data_ptr(), eps_d.data_ptr(), prior_d.data_ptr(), dz.data_ptr()
    dm = None
    if dmulv is not None:
        dm = dmulv.to(**f).contiguous()
        a.dmulv = dm.data_ptr()
    if prior_gen is not None:
        a.prior_gen, a.prior_step, a.prior_seed = 1, prior_gen[0].data_ptr(), prior_gen[1]
    nbytes, tiles = L.mmd_workspace(a)
    assert nbytes == tiles * 32 and tiles == (B + 15) // 16
    ws = torch.full((tiles * 4,), float("nan"), dtype=torch.float64, device=dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    st = L.stream_ptr()
    L.call("vae_mmd_fwd", ctypes.byref(a), st)
    # the consumer: vae_elbo_fwd, loss = 0*recon + 0*kld + 1*mmd
    sse, out, per, hc, kc, mo = (torch.zeros(n, **f) for n in (B, 4, B, B, B, 1))
    e = L.ElboArgs(kind=L.LOSS_INFO, batch=B, samples=1, latent=D, img_elems=1, kld_weight=0.0,
                   recon_weight=0.0, kl_factor=0.0, mmd_coef=1.0, mmd_tiles=tiles)
    e.mulv, e.sse, e.out, e.per_img, e.head_coef, e.kl_coef = (t.data_ptr() for t in (mulv_d, sse, out, per, hc, kc))
    e.mmd_partials, e.mmd_out = ws.data_ptr(), mo.data_ptr()
    L.call("vae_elbo_fwd", ctypes.byref(e), st)
    torch.cuda.synchronize()
    assert float(out[0]) == float(mo[0])
    return dict(mmd=float(mo[0]), dz=dz.cpu(), partials=ws.cpu(), prior=prior_d.cpu(),
                dmulv=None if dm is None else dm.cpu())


def ref_mmd(mulv, eps, prior, kind, latent_var=2.0, dtype=torch.float64):
    """(mmd, dmmd/dz, dmmd/dmulv) of the restated reference in `dtype`."""
    D = eps.shape[1]
    mv = mulv.to(dtype).clone().requires_grad_(True)
    z = mv[:, :D] + eps.to(dtype) * torch.exp(0.5 * mv[:, D:])
    z.retain_grad()
    m = R.compute_mmd(z, prior.to(dtype), kind, latent_var)
    m.backward()
    return float(m.detach()), z.grad.detach(), mv.grad.detach()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@pytest.mark.parametrize("kind", ["imq", "rbf"])
@pytest.mark.parametrize("D", [32, 128, 256])
@pytest.mark.parametrize("B", [2, 4, 16, 24, 48, 64, 144])
def test_mmd_and_gradient_match_fp64(B, D, kind):
    mulv, eps, prior = _inputs(B, D)
    got = run_mmd(mulv, eps, prior, kind)
    m64, dz64, _ = ref_mmd(mulv, eps, prior, kind)
    m32, dz32, _ = ref_mmd(mulv, eps, prior, kind, dtype=torch.float32)
    e_m, e_dz = abs(got["mmd"] - m64) / abs(m64), _rel(got["dz"], dz64)
    print(f"mmd {kind} B={B} D={D}: mmd {got['mmd']:.8g} fp64 {m64:.8g}; rel err hip {e_m:.2e} torch-fp32 "
          f"{abs(m32 - m64) / abs(m64):.2e}; dz rel-norm err hip {e_dz:.2e} torch-fp32 {_rel(dz32, dz64):.2e}")
    assert e_m <= 1e-4, (got["mmd"], m64)
    assert e_dz <= 1e-4
    assert bool(torch.isfinite(got["partials"]).all())


@pytest.mark.parametrize("kind", ["imq", "rbf"])
def test_grad_scale_and_dmulv_accumulate_onto_a_nonzero_buffer(kind):
    B, D, scale = 24, 128, 0.37
    mulv, eps, prior = _inputs(B, D, seed=1)
    _, dz64, dmv64 = ref_mmd(mulv, eps, prior, kind)
    want = scale * dmv64
    base = torch.randn(B, 2 * D, generator=torch.Generator().manual_seed(5)) * float(want.pow(2).mean().sqrt())
    got = run_mmd(mulv, eps, prior, kind, grad_scale=scale, dmulv=base)
    assert _rel(got["dz"], scale * dz64) <= 1e-4
    # the increment against fp64; base is of the increment's size, so its fp32 rounding (6e-8
    # relative) stays far below the bar
    assert _rel(got["dmulv"].double() - base.double(), want) <= 1e-4
    assert not torch.equal(got["dmulv"], base)


@pytest.mark.parametrize("kind", ["imq", "rbf"])
def test_reseed_adds_the_scaled_reparameterization_backward(kind):
    from vae_amd import _lib as L
    B, D, scale = 24, 128, -2.5
    mulv, eps, prior = _inputs(B, D, seed=2)
    _, _, dmv64 = ref_mmd(mulv, eps, prior, kind)
    got = run_mmd(mulv, eps, prior, kind)
    base = torch.randn(B, 2 * D, generator=torch.Generator().manual_seed(6)) * float((scale * dmv64).pow(2).mean().sqrt())
    dm, dz, s = base.cuda(), got["dz"].cuda(), torch.tensor([scale], device="cuda")
    mulv_d, eps_d = mulv.cuda(), eps.cuda()
    L.call("vae_mmd_reseed", B, D, dz.data_ptr(), s.data_ptr(), mulv_d.data_ptr(), eps_d.data_ptr(), dm.data_ptr(),
           L.stream_ptr())
    torch.cuda.synchronize()
    assert _rel(dm.cpu().double() - base.double(), scale * dmv64) <= 1e-4


@pytest.mark.parametrize("kind", ["imq", "rbf"])
def test_latents_equal_to_the_prior_give_zero(kind):
    """z == prior: the three matrices are the same numbers, so mmd is 0 up to the rounding of terms
    that are each computed to well within 1e-5 relative in fp32."""
    B, D = 48, 128
    _, _, prior = _inputs(B, D, seed=3)
    mulv = torch.cat([prior, torch.zeros(B, D)], 1)          # mu = prior, eps = 0: z = prior exactly
    got = run_mmd(mulv, torch.zeros(B, D), prior, kind)
    p = got["partials"].view(-1, 4).sum(0)
    assert abs(got["mmd"]) <= 1e-5 * float(p[0] + p[1] + 2 * p[2]), (got["mmd"], p)


@pytest.mark.parametrize("kind", ["imq", "rbf"])
def test_identical_rows_count_only_the_true_diagonal_is_dropped(kind):
    """Two equal latent rows: their off-diagonal pair has d^2 = 0 and k = 1 and must be counted
    (twice); dropping entries by value instead of by index would lose 2 from S_zz (imq)."""
    B, D = 4, 32
    mulv, eps, prior = _inputs(B, D, seed=4)
    mulv[1], eps[1] = mulv[0], eps[0]
    got = run_mmd(mulv, eps, prior, kind)
    m64, dz64, _ = ref_mmd(mulv, eps, prior, kind)
    assert abs(got["mmd"] - m64) <= 1e-4 * abs(m64), (got["mmd"], m64)
    assert _rel(got["dz"], dz64) <= 1e-4


@pytest.mark.parametrize("kind,B,D", [("imq", 64, 128), ("rbf", 144, 256)])
def test_two_calls_are_bit_identical(kind, B, D):
    mulv, eps, prior = _inputs(B, D, seed=5)
    a, b = run_mmd(mulv, eps, prior, kind), run_mmd(mulv, eps, prior, kind)
    assert a["mmd"] == b["mmd"]
    assert torch.equal(a["dz"], b["dz"]) and torch.equal(a["partials"], b["partials"])


def test_device_prior_is_standard_normal_fresh_per_step_and_repeatable():
    """prior_gen = 1 (Philox4x32-10 + Box-Muller keyed by (seed, *step)): N(0,1) moments and a
    Kolmogorov-Smirnov test, a fresh draw for another step, the same draw for the same (seed, step),
    and the value used inside the kernel is the one written out (mmd equals the run that reads it)."""
    import numpy as np
    from scipy import stats
    B, D = 512, 128
    mulv, eps, _ = _inputs(B, D, seed=6)
    step = torch.ones(1, dtype=torch.int32, device="cuda")
    draws, runs = [], []
    for s in (1, 2, 3):
        step.fill_(s)
        runs.append(run_mmd(mulv, eps, None, "imq", prior_gen=(step, 77)))
        draws.append(runs[-1]["prior"].double().flatten())
    for e in draws:
        assert e.numel() == B * D
        assert abs(float(e.mean())) < 0.03 and abs(float(e.std()) - 1) < 0.03, (float(e.mean()), float(e.std()))
        assert stats.kstest(e.numpy(), "norm").pvalue > 1e-4
        assert float(e.abs().max()) < 7.0 and bool(torch.isfinite(e).all())
    for a, b in zip(draws, draws[1:]):
        assert not torch.equal(a, b)
        assert abs(float(np.corrcoef(a.numpy(), b.numpy())[0, 1])) < 0.03
    step.fill_(1)
    again = run_mmd(mulv, eps, None, "imq", prior_gen=(step, 77))
    assert torch.equal(again["prior"], runs[0]["prior"]) and again["mmd"] == runs[0]["mmd"]
    other_seed = run_mmd(mulv, eps, None, "imq", prior_gen=(step, 78))
    assert not torch.equal(other_seed["prior"], runs[0]["prior"])
    # teacher-forced: reading the written draw gives the same numbers bit for bit
    read = run_mmd(mulv, eps, runs[0]["prior"], "imq")
    assert read["mmd"] == runs[0]["mmd"] and torch.equal(read["dz"], runs[0]["dz"])
