"""DIPVAE on the registry, the torch fallback of its loss_function and the C ABI of its covariance
kernel, without a GPU (models/dip_vae.py:8-21, :125-164; include/vaehip.h vae_dip_args, vae_elbo_args)."""
import ctypes
import inspect

import pytest
import torch

import dipvae_ref as R
from vae_amd import _lib as L


def test_registry_entry_is_the_model_class():
    from vae_amd import models
    assert models.vae_models['DIPVAE'] is models.DIPVAE
    assert issubclass(models.DIPVAE, models.BaseVAE)


def test_constructor_has_the_reference_arguments():
    from vae_amd import models
    sig = inspect.signature(models.vae_models['DIPVAE'].__init__)
    for k, v in {"lambda_diag": 10., "lambda_offdiag": 5.}.items():
        assert k in sig.parameters, k
        assert sig.parameters[k].default == v, k
    assert list(sig.parameters)[1:4] == ["in_channels", "latent_dim", "hidden_dims"]


def test_the_off_path_message_names_the_model():
    from vae_amd import models
    with pytest.raises(NotImplementedError, match="DIPVAE"):
        models.vae_models['WAE_MMD'](in_channels=3, latent_dim=128)


@pytest.mark.parametrize("B,D", [(1, 32), (8, 128), (40, 32)])
def test_torch_fallback_equals_the_restatement(B, D):
    """loss_function on foreign CPU tensors is the reference formula in torch: B = 1 (test_step scores
    images one by one), and more rows than latent dimensions."""
    from vae_amd import models
    g = torch.Generator().manual_seed(B + D)
    recons, x = torch.rand(B, 3, 8, 8, generator=g), torch.rand(B, 3, 8, 8, generator=g)
    mu = (0.5 * torch.randn(B, D, generator=g)).requires_grad_(True)
    lv = (0.3 * torch.randn(B, D, generator=g)).requires_grad_(True)
    lf = models.DIPVAE.loss_function
    stub = type("Stub", (), dict(lambda_diag=0.05, lambda_offdiag=0.1, _last=None))()
    got = lf(stub, recons, x, mu, lv, M_N=0.7)
    want = R.dip_loss(recons, x, mu, lv, 0.7, lambda_diag=0.05, lambda_offdiag=0.1)
    assert tuple(got) == R.TERMS
    for k in R.TERMS:
        assert float(got[k].detach()) == pytest.approx(float(want[k].detach()), rel=1e-6), k
    gm, gl = torch.autograd.grad(got["loss"], (mu, lv))
    wm, wl = torch.autograd.grad(want["loss"], (mu, lv))
    assert torch.allclose(gm, wm, rtol=1e-5, atol=1e-6) and torch.allclose(gl, wl, rtol=1e-5, atol=1e-6)


def test_struct_sizes_match_the_header_layout():
    # vae_dip_args: 6 x 4 bytes, 4 pointers, int64
    assert ctypes.sizeof(L.DipArgs) == 6 * 4 + 4 * 8 + 8
    assert L.DipArgs.mulv.offset == 24 and L.DipArgs.workspace_bytes.offset == 56
    # VAE_LOSS_DIP reads its partials through vae_elbo_args' tile fields: the struct keeps its size
    assert ctypes.sizeof(L.ElboArgs) == 144 and L.ElboArgs.mmd_out.offset == 136
    assert L.LOSS_DIP == 6
    assert {"vae_dip_fwd", "vae_dip_workspace_size"} <= set(L.EXPORTED)


def test_workspace_query_needs_no_device():
    for B, D in ((1, 32), (7, 32), (64, 128), (1024, 256)):
        a = L.DipArgs(batch=B, latent=D)
        tiles = D // 16
        assert L.dip_workspace(a) == (tiles * 2 * 8 + tiles * B * 4, tiles)


def _rc(a):
    lib = L.load()
    out = ctypes.c_size_t(0)
    q = lib.vae_dip_workspace_size(ctypes.byref(a), ctypes.byref(out), None)
    f = lib.vae_dip_fwd(ctypes.byref(a), None)
    return q, f, lib.vae_last_error()


def test_bad_shapes_return_their_own_reason_before_any_launch():
    ok = dict(batch=16, latent=128)
    reasons = set()
    for bad, word in ((dict(latent=48), b"multiple of 32"), (dict(latent=288), b"above 256"),
                      (dict(batch=0), b"below 1"), (dict(batch=1025), b"above 1024")):
        q, f, msg = _rc(L.DipArgs(**dict(ok, **bad)))
        assert q == -2 and f == -2 and word in msg, (bad, q, f, msg)
        reasons.add(msg)
    assert len(reasons) == 4
    # a good shape with null tensors: BADARG from the call, the query succeeds
    q, f, msg = _rc(L.DipArgs(**ok))
    assert q == 0 and f == -1 and b"dip_fwd" in msg
    # a misaligned mulv, a short workspace
    a = L.DipArgs(**ok)
    a.mulv, a.dmulv_dip, a.workspace, a.workspace_bytes = (1 << 20) + 4, 1 << 20, 1 << 20, 1 << 16
    assert _rc(a)[1] == -1 and b"aligned" in L.load().vae_last_error()
    a.mulv, a.workspace_bytes = 1 << 20, 64
    assert _rc(a)[1] == -1 and b"workspace" in L.load().vae_last_error()


def test_elbo_dip_kind_needs_its_partials():
    lib = L.load()
    e = L.ElboArgs(kind=L.LOSS_DIP, batch=16, samples=1, latent=128, img_elems=12288)
    e.sse = e.out = e.per_img = e.mulv = e.head_coef = e.kl_coef = 1 << 20
    assert lib.vae_elbo_fwd(ctypes.byref(e), None) == -1 and b"dip" in lib.vae_last_error()
    e.mmd_partials = e.mmd_out = 1 << 20
    e.mmd_tiles, e.samples = 8, 5
    assert lib.vae_elbo_fwd(ctypes.byref(e), None) == -2
    e7 = L.ElboArgs(kind=7, batch=16, samples=1, latent=128, img_elems=12288)
    e7.sse = e7.out = e7.per_img = 1 << 20
    assert lib.vae_elbo_fwd(ctypes.byref(e7), None) == -1
