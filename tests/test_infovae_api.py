"""InfoVAE on the registry and the C ABI of its MMD kernel, without a GPU (models/info_vae.py:8-31;
include/vaehip.h vae_mmd_args, vae_elbo_args)."""
import ctypes
import inspect

import pytest

from vae_amd import _lib as L


def test_registry_entry_is_the_model_class():
    from vae_amd import models
    assert models.vae_models['InfoVAE'] is models.InfoVAE
    assert issubclass(models.InfoVAE, models.BaseVAE)


def test_constructor_has_the_reference_arguments():
    from vae_amd import models
    sig = inspect.signature(models.vae_models['InfoVAE'].__init__)
    want = {"alpha": -0.5, "beta": 5.0, "reg_weight": 100, "kernel_type": 'imq', "latent_var": 2.}
    for k, v in want.items():
        assert k in sig.parameters, k
        assert sig.parameters[k].default == v, k
    assert list(sig.parameters)[1:3] == ["in_channels", "latent_dim"]


def test_positive_alpha_is_rejected_before_any_device_work():
    from vae_amd import models
    with pytest.raises(AssertionError, match="alpha must be negative or zero"):
        models.InfoVAE(3, 128, alpha=0.5)


def test_struct_sizes_match_the_header_layout():
    # vae_mmd_args: 6 x 4 bytes, 6 pointers, int64, pointer, uint64
    assert ctypes.sizeof(L.MmdArgs) == 6 * 4 + 6 * 8 + 8 + 8 + 8
    assert L.MmdArgs.mulv.offset == 24 and L.MmdArgs.prior_seed.offset == 88
    # vae_elbo_args: the round-6 layout (112 bytes) + 3 floats, int32, 2 pointers
    assert ctypes.sizeof(L.ElboArgs) == 112 + 4 * 4 + 2 * 8
    assert L.ElboArgs.recon_weight.offset == 112 and L.ElboArgs.mmd_partials.offset == 128
    assert L.LOSS_INFO == 5 and L.ABI_VERSION == 26


def test_workspace_query_needs_no_device():
    for B, tiles in ((2, 1), (16, 1), (17, 2), (64, 4), (1024, 64)):
        a = L.MmdArgs(kind=L.MMD_IMQ, batch=B, latent=128, latent_var=2.0)
        assert L.mmd_workspace(a) == (tiles * 4 * 8, tiles)


def _rc(a):
    lib = L.load()
    out = ctypes.c_size_t(0)
    q = lib.vae_mmd_workspace_size(ctypes.byref(a), ctypes.byref(out), None)
    f = lib.vae_mmd_fwd(ctypes.byref(a), None)
    return q, f, lib.vae_last_error()


def test_bad_shapes_and_arguments_return_their_codes_before_any_launch():
    ok = dict(kind=L.MMD_IMQ, batch=16, latent=128, latent_var=2.0)
    for bad, code in ((dict(batch=1), -2), (dict(batch=0), -2), (dict(batch=1025), -2), (dict(latent=48), -2),
                      (dict(latent=288), -2), (dict(latent=0), -2), (dict(kind=2), -1), (dict(kind=-1), -1),
                      (dict(latent_var=0.0), -1)):
        q, f, msg = _rc(L.MmdArgs(**dict(ok, **bad)))
        assert q == code and f == code, (bad, q, f, msg)
    # a good shape with null tensors: BADARG from the call, the query succeeds
    q, f, msg = _rc(L.MmdArgs(**ok))
    assert q == 0 and f == -1 and b"mmd_fwd" in msg
    # misaligned tensors, a short workspace, prior_gen without a step counter
    a = L.MmdArgs(**ok)
    a.mulv, a.eps, a.prior, a.dz, a.workspace, a.workspace_bytes = 1 << 20, (1 << 20) + 4, 1 << 20, 1 << 20, 1 << 20, 32
    assert _rc(a)[1] == -1
    a.eps, a.workspace_bytes = 1 << 20, 8
    assert _rc(a)[1] == -1 and b"workspace" in L.load().vae_last_error()
    a.workspace_bytes, a.prior_gen = 32, 1
    assert _rc(a)[1] == -1 and b"prior_step" in L.load().vae_last_error()
    lib = L.load()
    assert lib.vae_mmd_reseed(16, 128, None, None, None, None, None, None) == -1


def test_elbo_info_kind_needs_its_partials():
    lib = L.load()
    e = L.ElboArgs(kind=L.LOSS_INFO, batch=16, samples=1, latent=128, img_elems=12288)
    e.sse = e.out = e.per_img = e.mulv = e.head_coef = e.kl_coef = 1 << 20
    assert lib.vae_elbo_fwd(ctypes.byref(e), None) == -1 and b"mmd" in lib.vae_last_error()
    e.mmd_partials = e.mmd_out = 1 << 20
    e.mmd_tiles, e.batch = 1, 1
    assert lib.vae_elbo_fwd(ctypes.byref(e), None) == -2
    e6 = L.ElboArgs(kind=6, batch=16, samples=1, latent=128, img_elems=12288)
    e6.sse = e6.out = e6.per_img = 1 << 20
    assert lib.vae_elbo_fwd(ctypes.byref(e6), None) == -1
