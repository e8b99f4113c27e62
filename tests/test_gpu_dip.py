"""vae_dip_fwd (csrc/vae_dip.hip) against the reference's DIP term (models/dip_vae.py:146-158, restated
in tests/dipvae_ref.py) in fp64 torch with autograd.

Bars: dip within 1e-4 relative of fp64 (the project's fp32 loss bar), d dip/d mu and d dip/d log_var
each within 1e-4 relative norm of the fp64 gradient.  Each case prints fp32 torch's own distance from
fp64 (<= 4e-7 on these input scales, mu ~ 0.5 N, log_var ~ 0.3 N), so the margin is on record.
The dip value is read the way a step reads it: vae_elbo_fwd (VAE_LOSS_DIP) adds the partials.

Shapes: B = 1 (a one-row Gram matrix), 2, 7 (a ragged k-step of the batch product), 16, 24, 40 (more
rows than a 32-row chunk; more rows than D = 32), 64 (the config's batch; exactly one 64-row chunk),
144 (several chunks, the last ragged); D = 32 (two strips, two of the four waves idle in the first
product), 128 (64-row chunks; B <= 64 keeps its one chunk in LDS for the second product) and 256
(32-row chunks, four 16-row tiles of the strip per wave in the first product)."""
import ctypes

import pytest
import torch

import dipvae_ref as R

pytestmark = pytest.mark.gpu

LAMBDAS = [(0.1, 0.05), (5.0, 10.0)]            # (lambda_offdiag, lambda_diag): the yaml's, the defaults'


def _inputs(B, D, seed=0):
    g = torch.Generator().manual_seed(1000 * B + D + seed)
    return torch.cat([0.5 * torch.randn(B, D, generator=g), 0.3 * torch.randn(B, D, generator=g)], 1)


def run_dip(mulv, l_off, l_diag, grad_scale=1.0, dmulv=None):
    """One vae_dip_fwd + the consumer's ordered sum.  Returns dict(dip, g, ws, dmulv); the outputs
    and the workspace start NaN-filled."""
    from vae_amd import _lib as L
    B, D = mulv.shape[0], mulv.shape[1] // 2
    f = dict(dtype=torch.float32, device="cuda")
    mulv_d = mulv.to(**f).contiguous()
    g = torch.full((B, 2 * D), float("nan"), **f)
    a = L.DipArgs(batch=B, latent=D, lambda_diag=l_diag, lambda_offdiag=l_off, grad_scale=grad_scale)
    a.mulv, a.dmulv_dip = mulv_d.data_ptr(), g.data_ptr()
    dm = None
    if dmulv is not None:
        dm = dmulv.to(**f).contiguous()
        a.dmulv = dm.data_ptr()
    nbytes, tiles = L.dip_workspace(a)
    assert tiles == D // 16 and nbytes == tiles * 16 + tiles * B * 4
    # (the workspace as 4-byte words, so that its float tail is exactly as long as the query says)
    ws = torch.full((nbytes // 4,), float("nan"), **f)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    st = L.stream_ptr()
    L.call("vae_dip_fwd", ctypes.byref(a), st)
    # the consumer: vae_elbo_fwd, loss = 0 (sse) + 0 * kld + dip
    sse, out, per, hc, kc, do = (torch.zeros(n, **f) for n in (B, 4, B, B, B, 1))
    e = L.ElboArgs(kind=L.LOSS_DIP, batch=B, samples=1, latent=D, img_elems=1, kld_weight=0.0, mmd_tiles=tiles)
    e.mulv, e.sse, e.out, e.per_img, e.head_coef, e.kl_coef = (t.data_ptr() for t in (mulv_d, sse, out, per, hc, kc))
    e.mmd_partials, e.mmd_out = ws.data_ptr(), do.data_ptr()
    L.call("vae_elbo_fwd", ctypes.byref(e), st)
    torch.cuda.synchronize()
    assert float(out[0]) == float(do[0])
    assert bool((hc == 2.0).all()) and bool((kc == 0.0).all())
    ws = ws.cpu()
    return dict(dip=float(do[0]), g=g.cpu(), ws=ws, partials=ws[:4 * tiles].view(torch.float64),
                rowsum=ws[4 * tiles:], dmulv=None if dm is None else dm.cpu())


def ref_dip(mulv, l_off, l_diag, dtype=torch.float64):
    D = mulv.shape[1] // 2
    mv = mulv.to(dtype).clone().requires_grad_(True)
    d = R.dip_term(mv[:, :D], mv[:, D:], l_diag, l_off)
    d.backward()
    return float(d.detach()), mv.grad.detach()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("D", [32, 128, 256])
@pytest.mark.parametrize("B", [1, 2, 7, 16, 24, 40, 64, 144])
def test_dip_and_gradient_match_fp64(B, D, lam):
    mulv = _inputs(B, D)
    got = run_dip(mulv, *lam)
    d64, g64 = ref_dip(mulv, *lam)
    d32, g32 = ref_dip(mulv, *lam, dtype=torch.float32)
    e_d = abs(got["dip"] - d64) / abs(d64)
    e_mu, e_lv = _rel(got["g"][:, :D], g64[:, :D]), _rel(got["g"][:, D:], g64[:, D:])
    print(f"dip B={B} D={D} lambdas={lam}: dip {got['dip']:.8g} fp64 {d64:.8g}; rel err hip {e_d:.2e} torch-fp32 "
          f"{abs(d32 - d64) / abs(d64):.2e}; dmu rel-norm err hip {e_mu:.2e} torch-fp32 {_rel(g32[:, :D], g64[:, :D]):.2e}; "
          f"dlog_var hip {e_lv:.2e} torch-fp32 {_rel(g32[:, D:], g64[:, D:]):.2e}")
    assert e_d <= 1e-4, (got["dip"], d64)
    assert e_mu <= 1e-4
    assert e_lv <= 1e-4
    # NaN-filled outputs and workspace are fully overwritten
    # (the workspace read as what it holds: [tiles][2] doubles, then [tiles][B] floats)
    assert bool(torch.isfinite(got["g"]).all())
    assert bool(torch.isfinite(got["partials"]).all()) and bool(torch.isfinite(got["rowsum"]).all())
    assert got["partials"].numel() == 2 * (D // 16) and got["rowsum"].numel() == (D // 16) * B


def test_rows_beyond_the_latent_size_get_no_log_var_gradient():
    B, D = 40, 32
    got = run_dip(_inputs(B, D, seed=1), 0.1, 0.05)
    glv = got["g"][:, D:]
    assert bool((glv[D:] == 0).all())                              # rows >= D: exactly zero
    off = glv[:D].clone()
    off[torch.arange(D), torch.arange(D)] = 0
    assert bool((off == 0).all())                                  # off the diagonal: exactly zero
    assert bool((torch.diagonal(glv[:D]) != 0).all())


def test_short_batch_seeds_only_its_own_diagonal():
    B, D = 7, 32
    got = run_dip(_inputs(B, D, seed=2), 5.0, 10.0)
    glv = got["g"][:, D:]
    mask = torch.zeros(B, D, dtype=torch.bool)
    mask[torch.arange(B), torch.arange(B)] = True
    assert bool((glv[~mask] == 0).all()) and bool((glv[mask] != 0).all())


def test_grad_scale_and_dmulv_accumulate_onto_a_nonzero_buffer():
    B, D, scale = 24, 128, 0.37
    mulv = _inputs(B, D, seed=3)
    _, g64 = ref_dip(mulv, 0.1, 0.05)
    want = scale * g64
    base = torch.randn(B, 2 * D, generator=torch.Generator().manual_seed(5)) * float(want[:, :D].pow(2).mean().sqrt())
    got = run_dip(mulv, 0.1, 0.05, grad_scale=scale, dmulv=base)
    assert _rel(got["g"], want) <= 1e-4
    # the increment against fp64; base is of the mu increment's size, so its fp32 rounding (6e-8
    # relative) stays far below the bar
    assert _rel(got["dmulv"].double() - base.double(), want) <= 1e-4
    assert not torch.equal(got["dmulv"], base)
    # without dmulv nothing else is written, and grad_scale 1 gives the unscaled gradient
    assert _rel(run_dip(mulv, 0.1, 0.05)["g"], g64) <= 1e-4


@pytest.mark.parametrize("B,D", [(64, 128), (144, 256)])
def test_two_calls_are_bit_identical(B, D):
    mulv = _inputs(B, D, seed=4)
    a, b = run_dip(mulv, 0.1, 0.05), run_dip(mulv, 0.1, 0.05)
    assert a["dip"] == b["dip"]
    assert torch.equal(a["g"], b["g"])
    assert torch.equal(a["partials"], b["partials"]) and torch.equal(a["rowsum"], b["rowsum"])
