"""MIWAE on the registry, the torch fallback of its loss_function, the C ABI of VAE_LOSS_MIWAE and
StepPlan's argument checks, without a GPU (models/miwae.py:8-30, :132-164; include/vaehip.h
vae_elbo_args)."""
import ctypes
import inspect

import pytest
import torch

import miwae_ref as R
from vae_amd import _lib as L


def test_registry_entry_is_the_model_class():
    from vae_amd import models
    assert models.vae_models['MIWAE'] is models.MIWAE
    assert issubclass(models.MIWAE, models.BaseVAE)


def test_constructor_has_the_reference_arguments():
    from vae_amd import models
    sig = inspect.signature(models.vae_models['MIWAE'].__init__)
    for k, v in {"num_samples": 5, "num_estimates": 5}.items():
        assert k in sig.parameters, k
        assert sig.parameters[k].default == v, k
    assert list(sig.parameters)[1:6] == ["in_channels", "latent_dim", "hidden_dims", "num_samples", "num_estimates"]


def test_the_off_path_message_names_the_model():
    from vae_amd import models
    with pytest.raises(NotImplementedError, match="MIWAE"):
        models.vae_models['WAE_MMD'](in_channels=3, latent_dim=128)
    with pytest.raises(NotImplementedError, match="DIPVAE"):
        models.vae_models['WAE_MMD'](in_channels=3, latent_dim=128)


@pytest.mark.parametrize("B,M,K", [(1, 5, 5), (3, 2, 3), (2, 4, 1)])
def test_torch_fallback_equals_the_restatement(B, M, K):
    """loss_function on foreign CPU tensors is the reference formula in torch: values and autograd
    gradients, B = 1 (test_step scores images one by one) and K = 1 included."""
    from vae_amd import models
    g = torch.Generator().manual_seed(100 * B + 10 * M + K)
    D = 16
    recons = torch.rand(B, M, K, 3, 8, 8, generator=g).requires_grad_(True)
    x = torch.rand(B, 3, 8, 8, generator=g)
    mu = (0.5 * torch.randn(B, 1, 1, D, generator=g)).expand(B, M, K, D).clone().requires_grad_(True)
    lv = (0.3 * torch.randn(B, 1, 1, D, generator=g)).expand(B, M, K, D).clone().requires_grad_(True)
    stub = type("Stub", (), dict(num_samples=K, num_estimates=M, _last=None, training=True,
                                 _gpu_loss=lambda self, *a, **k: None))()
    got = models.MIWAE.loss_function(stub, recons, x, mu, lv, None, None, M_N=0.7)
    want = R.miwae_loss(recons, x, mu, lv, 0.7)
    assert tuple(got) == R.TERMS
    for k in R.TERMS:
        assert float(got[k].detach()) == pytest.approx(float(want[k].detach()), rel=1e-6), k
    gg = torch.autograd.grad(got["loss"], (recons, mu, lv))
    ww = torch.autograd.grad(want["loss"], (recons, mu, lv))
    for a, b in zip(gg, ww):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-8)
    # and the fp64 closed form the kernel implements, from the same rows
    sse = ((recons.detach() - x[:, None, None]) ** 2).flatten(3).sum(-1).reshape(-1)
    mulv = torch.cat([mu.detach()[:, 0, 0], lv.detach()[:, 0, 0]], 1)
    out64, _, hc, _ = R.miwae_elbo64(sse, mulv, M, K, 0.7, 3 * 8 * 8)
    assert float(got["loss"].detach()) == pytest.approx(float(out64[0]), rel=1e-5)
    # dL/drecon = head_coef * (recon - x)
    seed = hc.view(B, M, K, 1, 1, 1) * (recons.detach() - x[:, None, None]).double()
    assert float((gg[0].double() - seed).norm() / seed.norm()) < 1e-5


def test_abi_is_unchanged_and_the_kind_is_seven():
    assert L.LOSS_MIWAE == 7
    assert ctypes.sizeof(L.ElboArgs) == 144 and L.ElboArgs.mmd_out.offset == 136
    assert L.ABI_VERSION == 26 and L.load().vae_abi_version() == 26


def _rc(**kw):
    """vae_elbo_fwd on a VAE_LOSS_MIWAE call with (fake, never dereferenced) tensors: (code, reason)."""
    lib = L.load()
    ok = dict(kind=L.LOSS_MIWAE, batch=4, samples=15, latent=128, img_elems=12288, mmd_tiles=3)
    null = kw.pop("null", ())
    e = L.ElboArgs(**dict(ok, **kw))
    for f in ("sse", "out", "per_img", "mulv", "head_coef", "kl_coef"):
        setattr(e, f, None if f in null else 1 << 20)
    return lib.vae_elbo_fwd(ctypes.byref(e), None), lib.vae_last_error()


def test_bad_shapes_return_their_own_reason_before_any_launch():
    reasons = set()
    for bad, word in ((dict(mmd_tiles=0), b"below 1"), (dict(mmd_tiles=-2), b"below 1"),
                      (dict(samples=16), b"multiple"), (dict(samples=2, mmd_tiles=3), b"multiple"),
                      (dict(batch=0), b"1..1024"), (dict(batch=1025), b"1..1024")):
        rc, msg = _rc(**bad)
        assert rc == -2 and word in msg and b"MIWAE" in msg, (bad, rc, msg)
        reasons.add(word)
    assert len(reasons) == 3
    # null tensors are BADARG, and are looked at before the shapes
    for f in ("mulv", "head_coef", "kl_coef", "sse", "out", "per_img"):
        assert _rc(null=(f,))[0] == -1, f
        assert _rc(null=(f,), mmd_tiles=0, batch=0)[0] == -1, f
    # kinds above MIWAE are still unknown
    for kind in (8, 9, 100):
        assert _rc(kind=kind)[0] == -1


def test_plan_argument_checks_need_no_device():
    from vae_amd.net import StepPlan, VAENet
    net = VAENet(latent_dim=64, dtype=torch.float32, device="cpu")
    assert StepPlan.LOSS_KINDS["miwae"] == L.LOSS_MIWAE
    for loss in ("vanilla", "betaH", "betaB", "iwae", "info", "dip"):
        with pytest.raises(ValueError, match="estimates"):
            StepPlan(net, 4, loss=loss, samples=5, estimates=1)
    for kw in (dict(samples=5, estimates=0), dict(samples=0, estimates=3), dict(samples=5, estimates=-1)):
        with pytest.raises(ValueError, match="samples >= 1 and estimates >= 1"):
            StepPlan(net, 4, loss="miwae", **kw)
    for B in (0, 1025):
        with pytest.raises(ValueError, match="1..1024"):
            StepPlan(net, B, loss="miwae", samples=5, estimates=3)


def test_model_holds_the_reference_attributes_and_keys():
    """Built on the CPU: no kernel runs in the constructor or in state_dict interop."""
    from oracle import vae_oracle as O
    from vae_amd import models
    m = models.MIWAE(3, 128, num_samples=5, num_estimates=3, device="cpu")
    assert (m.num_samples, m.num_estimates, m.samples) == (5, 3, 15)
    assert m._loss_config() == dict(loss="miwae", samples=5, estimates=3)
    spec = O.make_params(O.vanilla_param_spec(latent_dim=128), 3)
    m.load_reference_state_dict(spec)
    back = m.reference_state_dict()
    assert list(back) == list(spec)
    assert all(torch.equal(back[k].cpu(), spec[k]) for k in spec)
