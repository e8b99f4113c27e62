"""The DIP-VAE drop-in model (vae_amd.models.DIPVAE; models/dip_vae.py:8-191): the BaseVAE interface
on the HIP forward, loss_function on the GPU (vae_dip_fwd + vae_elbo_fwd) with the fused backward
seeded from it, and the torch formula on anything else."""
import functools

import pytest
import torch

import dipvae_ref as R
from golden_util import load_case

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case():
    meta, _ = load_case("dipvae_b16")
    sd, x, eps = R.case_inputs(meta)
    return meta, sd, x, eps, R.train_step(sd, x, eps, M_N=meta["M_N"], **R.loss_kwargs(meta))


def _model(meta, sd):
    from vae_amd.models import vae_models
    m = vae_models["DIPVAE"](**meta["ctor"], dtype=torch.float32, device="cuda")
    m.load_reference_state_dict(sd)
    return m.train()


def _step(model, meta, x, eps, scale=1.0, backwards=1):
    model.flat.grad = None
    out = model(x.cuda(), eps=eps.cuda())
    ld = model.loss_function(*out, M_N=meta["M_N"])
    loss = scale * ld["loss"]
    for i in range(backwards):
        loss.backward(retain_graph=i + 1 < backwards)
    torch.cuda.synchronize()
    return out, ld, model.flat.grad.clone()


def test_forward_list_loss_dict_and_backward_match_the_fused_plan():
    from test_gpu_dipvae_step import run_plan
    meta, sd, x, eps, ref = _case()
    model = _model(meta, sd)
    out, ld, g1 = _step(model, meta, x, eps)
    recons, inp, mu, log_var = out                       # dip_vae.py:123
    assert len(out) == 4 and torch.equal(inp.cpu(), x)
    assert recons.shape == x.shape and mu.shape == log_var.shape == (x.shape[0], 128)
    assert ld["loss"].grad_fn is not None and type(ld["loss"].grad_fn).__name__.startswith("_HipELBO")
    assert tuple(ld) == R.TERMS
    for k in R.TERMS:
        assert abs(float(ld[k].detach()) - ref["loss"][k]) <= 1e-4 * abs(ref["loss"][k]), (k, float(ld[k].detach()))
    # the same gradients as the fused plan (the same kernels, the same seeds).  Not asserted bit for
    # bit: the fused plan's vae_dip_fwd adds its gradient into dmulv itself, the drop-in path stores it
    # and adds it multiplied by dL/dloss, and its head / KL seeds are products with dL/dloss too — the
    # same values up to one fp32 rounding per seed element (6e-8), which the backward carries linearly;
    # 1e-6 relative norm allows ~16 such roundings.
    _, runs, _ = run_plan(sd, x, eps, torch.float32, meta["M_N"], **R.loss_kwargs(meta))
    fused = runs[0][1]
    assert float((g1 - fused).norm() / fused.norm()) <= 1e-6
    # loss * 0.37 scales every seed, the DIP one included
    _, _, gs = _step(model, meta, x, eps, scale=0.37)
    assert float((gs - 0.37 * g1).norm() / (0.37 * g1).norm()) <= 1e-6
    # a scaled loss by a power of two: exactly twice
    _, _, g2 = _step(model, meta, x, eps, scale=2.0)
    assert torch.equal(g2, 2 * g1)
    # a second backward of the same loss (reset_backward) accumulates the same gradient again
    _, _, g3 = _step(model, meta, x, eps, backwards=2)
    assert torch.equal(g3, g1 + g1)


def test_eval_and_foreign_tensors_take_the_torch_formula():
    meta, sd, x, eps, ref = _case()
    model = _model(meta, sd)
    kw = R.loss_kwargs(meta)
    # foreign tensors (clones of a training forward's outputs): the formula, differentiable
    out = model(x.cuda(), eps=eps.cuda())
    args = [t.detach().clone() for t in out]
    ld = model.loss_function(*args, M_N=meta["M_N"])
    want = R.dip_loss(*[t.cpu() for t in args], meta["M_N"], **kw)
    for k in R.TERMS:
        assert abs(float(ld[k]) - float(want[k])) <= 1e-5 * abs(float(want[k])), (k, float(ld[k]), float(want[k]))
    # eval mode: running-statistics BatchNorm, no autograd, the formula; the forward is the
    # restatement's eval forward
    # (a fresh model: the training forward above has moved the running statistics)
    model = _model(meta, sd).eval()
    with torch.no_grad():
        out = model(x.cuda(), eps=eps.cuda())
        ld = model.loss_function(*out, M_N=meta["M_N"])
    assert len(out) == 4 and not out[0].requires_grad and ld["loss"].grad_fn is None
    ev = R.train_step(sd, x, eps, M_N=meta["M_N"], training=False, **kw)
    torch.testing.assert_close(out[2].cpu(), ev["mu"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(out[3].cpu(), ev["log_var"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(out[0].cpu(), ev["recon"], rtol=1e-4, atol=1e-5)
    want = R.dip_loss(*[t.cpu() for t in out], meta["M_N"], **kw)
    for k in R.TERMS:
        assert abs(float(ld[k]) - float(want[k])) <= 1e-5 * abs(float(want[k])), (k, float(ld[k]), float(want[k]))
        assert abs(float(ld[k]) - ev["loss"][k]) <= 1e-4 * abs(ev["loss"][k]), (k, float(ld[k]), ev["loss"][k])


def test_reference_keyed_state_dict_round_trip():
    meta, sd, *_ = _case()
    model = _model(meta, sd)
    got = model.state_dict()
    assert list(got) == list(sd)
    for k, v in sd.items():
        assert torch.equal(got[k].cpu(), v), k
    from vae_amd.models import DIPVAE
    other = DIPVAE(3, 128, dtype=torch.float32, device="cuda")
    other.load_state_dict({k: v.clone() for k, v in got.items()}, strict=True)
    assert torch.equal(other.flat.detach(), model.flat.detach())


def test_eval_plan_with_a_fused_dip_loss_is_rejected_at_construction():
    """An eval plan builds no DIP call, so a fused VAE_LOSS_DIP ELBO would have no partials to add:
    the combination is an error when the plan is built, not when it runs."""
    from vae_amd.net import StepPlan, VAENet
    net = VAENet(latent_dim=128, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="fused_loss=False"):
        StepPlan(net, 8, loss="dip", training=False)
    plan = StepPlan(net, 8, loss="dip", training=False, fused_loss=False)
    assert plan.dip is None and not any(fn in ("vae_dip_fwd", "vae_elbo_fwd") for fn, _ in plan.fwd_calls)
