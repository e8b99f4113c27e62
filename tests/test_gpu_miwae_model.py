"""The MIWAE drop-in model (vae_amd.models.MIWAE; models/miwae.py:8-192): the BaseVAE interface on the
HIP forward at B*M*K decoder rows, loss_function on the GPU (vae_elbo_fwd, VAE_LOSS_MIWAE) with the
fused backward seeded from it, and the torch formula on anything else."""
import functools

import pytest
import torch

import miwae_ref as R
from golden_util import load_case

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case():
    meta, _ = load_case("miwae_b4")
    sd, x, eps = R.case_inputs(meta)
    M, K = R.case_mk(meta)
    return meta, sd, x, eps, M, K, R.train_step(sd, x, eps, M_N=meta["M_N"], M=M, K=K)


@functools.lru_cache(maxsize=None)
def _spread():
    """The restatement's own per-gradient spread on the case (parity_util.grad_bar's input)."""
    meta, sd, x, eps, M, K, _ = _case()
    return R.with_spread(sd, x, eps, M_N=meta["M_N"], M=M, K=K)[1]


def _model(meta, sd):
    from vae_amd.models import vae_models
    m = vae_models["MIWAE"](**meta["ctor"], dtype=torch.float32, device="cuda")
    m.load_reference_state_dict(sd)
    return m.train()


def _step(model, M_N, x, eps, scale=1.0, backwards=1):
    model.flat.grad = None
    out = model(x.cuda(), eps=eps.cuda())
    ld = model.loss_function(*out, M_N=M_N)
    loss = scale * ld["loss"]
    for i in range(backwards):
        loss.backward(retain_graph=i + 1 < backwards)
    torch.cuda.synchronize()
    return out, ld, model.flat.grad.clone()


def test_forward_list_loss_dict_and_backward_match_the_fused_plan():
    from test_gpu_miwae_step import run_plan
    meta, sd, x, eps, M, K, ref = _case()
    B, D = x.shape[0], 128
    model = _model(meta, sd)
    out, ld, g1 = _step(model, meta["M_N"], x, eps)
    recons, inp, mu, log_var, z, eps_ret = out             # miwae.py:130
    assert len(out) == 6 and torch.equal(inp.cpu(), x)
    assert recons.shape == (B, M, K, 3, 64, 64)
    assert mu.shape == log_var.shape == z.shape == eps_ret.shape == (B, M, K, D)
    # rows in b, m, k order: the reconstructions are the restatement's, mu is repeated over m and k
    assert float((recons.detach().cpu().reshape(ref["recon"].shape) - ref["recon"]).norm() / ref["recon"].norm()) <= 1e-4
    assert torch.equal(mu[:, 1, 2], mu[:, 0, 0]) and torch.equal(log_var[:, M - 1, K - 1], log_var[:, 0, 0])
    torch.testing.assert_close(mu[:, 0, 0].detach().cpu(), ref["mu"], rtol=1e-4, atol=1e-5)
    zz = eps.view(B, M, K, D) * torch.exp(0.5 * log_var.detach().cpu()) + mu.detach().cpu()
    torch.testing.assert_close(z.detach().cpu(), zz, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(eps_ret.detach().cpu(), (zz - mu.detach().cpu()) / log_var.detach().cpu(),
                               rtol=1e-3, atol=1e-3)        # miwae.py:129: divided by log_var, not std
    assert ld["loss"].grad_fn is not None and type(ld["loss"].grad_fn).__name__.startswith("_HipELBO")
    assert tuple(ld) == R.TERMS
    for k in R.TERMS:
        assert abs(float(ld[k].detach()) - ref["loss"][k]) <= 1e-4 * abs(ref["loss"][k]), (k, float(ld[k].detach()))
    # the same gradients as the fused plan (the same kernels, the same seeds), up to the one fp32
    # rounding per seed element of the drop-in's product with dL/dloss = 1.0 — which is exact
    _, runs, _ = run_plan(sd, x, eps, torch.float32, meta["M_N"], M, K)
    fused = runs[0][1]
    assert float((g1 - fused).norm() / fused.norm()) <= 1e-6
    # a scaled loss by a power of two: exactly twice; 0.37: every seed scaled
    _, _, g2 = _step(model, meta["M_N"], x, eps, scale=2.0)
    assert torch.equal(g2, 2 * g1)
    _, _, gs = _step(model, meta["M_N"], x, eps, scale=0.37)
    assert float((gs - 0.37 * g1).norm() / (0.37 * g1).norm()) <= 1e-6
    # a second backward of the same loss (reset_backward) accumulates the same gradient again
    _, _, g3 = _step(model, meta["M_N"], x, eps, backwards=2)
    assert torch.equal(g3, g1 + g1)


def test_autograd_through_the_torch_formula_gives_the_same_gradient():
    """Foreign tensors (clones that keep the graph: views of the forward's outputs) take the formula in
    torch, and its autograd backward through the drop-in's HIP backward is the GPU loss's gradient."""
    from parity_util import grad_bar
    meta, sd, x, eps, M, K, ref = _case()
    model = _model(meta, sd)
    model.flat.grad = None
    out = model(x.cuda(), eps=eps.cuda())
    args = [out[0] * 1.0, out[1], out[2] * 1.0, out[3] * 1.0, out[4], out[5]]
    ld = model.loss_function(*args, M_N=meta["M_N"])
    assert not type(ld["loss"].grad_fn).__name__.startswith("_HipELBO")
    for k in R.TERMS:
        assert abs(float(ld[k].detach()) - ref["loss"][k]) <= 1e-4 * abs(ref["loss"][k]), k
    ld["loss"].backward()
    torch.cuda.synchronize()
    grads = {k: v.cpu() for k, v in model.net.layout.export_reference(model.flat.grad).items()}
    for name, gr in ref["grads"].items():
        if R.pre_bn_bias(name):
            continue
        err = float((grads[name].double() - gr.double()).norm() / gr.double().norm())
        assert err < grad_bar(name, _spread()), (name, err, grad_bar(name, _spread()))


def test_eval_generate_sample_and_decode_shapes():
    meta, sd, x, eps, M, K, ref = _case()
    B = x.shape[0]
    model = _model(meta, sd).eval()
    ev = R.train_step(sd, x, eps, M_N=meta["M_N"], M=M, K=K, training=False)
    with torch.no_grad():
        out = model(x.cuda(), eps=eps.cuda())
        ld = model.loss_function(*out, M_N=meta["M_N"])
        assert out[0].shape == (B, M, K, 3, 64, 64) and not out[0].requires_grad and ld["loss"].grad_fn is None
        torch.testing.assert_close(out[0].cpu().reshape(ev["recon"].shape), ev["recon"], rtol=1e-4, atol=1e-5)
        for k in R.TERMS:
            assert abs(float(ld[k]) - ev["loss"][k]) <= 1e-4 * abs(ev["loss"][k]), (k, float(ld[k]), ev["loss"][k])
        gen = model.generate(x.cuda())
        assert gen.shape == x.shape
        smp = model.sample(7, "cuda")                      # [7,1,1,D] -> squeeze: [7,C,H,W]
        assert smp.shape == (7, 3, 64, 64) and bool(torch.isfinite(smp).all())
        one = model.sample(1, "cuda")                      # squeeze() drops the batch axis too, as the reference's
        assert one.shape == (3, 64, 64)
        dec = model.decode(torch.randn(2, M, K, 128, device="cuda"))
        assert dec.shape == (2, M, K, 3, 64, 64)
        # a decoded row does not depend on the plan that decoded it (eval-mode BatchNorm)
        z = torch.randn(2, M, K, 128, device="cuda")
        a = model.decode(z)
        b = model.decode(z.reshape(2 * M * K, 1, 1, 128)[:7])
        torch.testing.assert_close(b.reshape(7, 3, 64, 64), a.reshape(-1, 3, 64, 64)[:7], rtol=1e-5, atol=1e-6)


def test_reference_keyed_state_dict_round_trip():
    meta, sd, *_ = _case()
    model = _model(meta, sd)
    got = model.state_dict()
    assert list(got) == list(sd)
    for k, v in sd.items():
        assert torch.equal(got[k].cpu(), v), k
    from vae_amd.models import MIWAE
    other = MIWAE(3, 128, dtype=torch.float32, device="cuda")
    assert (other.num_samples, other.num_estimates) == (5, 5)
    other.load_state_dict({k: v.clone() for k, v in got.items()}, strict=True)
    assert torch.equal(other.flat.detach(), model.flat.detach())


def test_one_by_one_is_the_plain_elbo():
    """M = K = 1 is legal: one row per image, w = 1, the VanillaVAE loss on one sample."""
    from oracle import vae_oracle as O
    from vae_amd.models import MIWAE
    meta, sd, x, _, *_ = _case()
    eps = O.make_inputs(x.shape[0], 128, 9)[1]
    model = MIWAE(3, 128, num_samples=1, num_estimates=1, dtype=torch.float32, device="cuda").train()
    model.load_reference_state_dict(sd)
    out, ld, g = _step(model, 0.5, x, eps)
    assert out[0].shape == (x.shape[0], 1, 1, 3, 64, 64)
    ref = O.train_step("VanillaVAE", sd, x, eps, M_N=0.5, do_adam=False)
    for k in R.TERMS:
        assert abs(float(ld[k].detach()) - ref["loss"][k]) <= 1e-4 * abs(ref["loss"][k]), (k, float(ld[k].detach()))
    grads = {k: v.cpu() for k, v in model.net.layout.export_reference(g).items()}
    for name in ("fc_mu.weight", "encoder.2.0.weight", "decoder.1.0.weight", "final_layer.3.weight"):
        gr = ref["grads"][name]
        assert float((grads[name] - gr).norm() / gr.norm()) < 1e-3, name
