"""The InfoVAE drop-in model (vae_amd.models.InfoVAE; models/info_vae.py:8-256): the BaseVAE
interface on the HIP forward, loss_function on the GPU (vae_mmd_fwd + vae_elbo_fwd) with the fused
backward seeded from it, and the torch formula on anything else."""
import functools

import pytest
import torch

import infovae_ref as R
from infovae_golden import TERMS, case_inputs, load_case, loss_kwargs

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case():
    meta, _ = load_case("infovae_imq_b16")
    sd, x, eps, prior = case_inputs(meta)
    return meta, sd, x, eps, prior, R.train_step(sd, x, eps, prior, M_N=meta["M_N"], **loss_kwargs(meta))


def _model(meta, sd):
    from vae_amd.models import vae_models
    m = vae_models["InfoVAE"](**meta["ctor"], dtype=torch.float32, device="cuda")
    m.load_reference_state_dict(sd)
    return m.train()


def _step(model, meta, x, eps, prior, scale=1.0, backwards=1):
    model.flat.grad = None
    out = model(x.cuda(), eps=eps.cuda())
    ld = model.loss_function(*out, M_N=meta["M_N"], prior=prior.cuda())
    loss = scale * ld["loss"]
    for i in range(backwards):
        loss.backward(retain_graph=i + 1 < backwards)
    torch.cuda.synchronize()
    return out, ld, model.flat.grad.clone()


def test_forward_list_loss_dict_and_backward_match_the_fused_plan():
    from test_gpu_infovae_step import run_plan
    meta, sd, x, eps, prior, ref = _case()
    model = _model(meta, sd)
    out, ld, g1 = _step(model, meta, x, eps, prior)
    recons, inp, z, mu, log_var = out                    # info_vae.py:126
    assert len(out) == 5 and torch.equal(inp.cpu(), x)
    assert recons.shape == x.shape and z.shape == mu.shape == log_var.shape == (x.shape[0], 128)
    torch.testing.assert_close(z.detach().cpu(), mu.detach().cpu() + eps * torch.exp(0.5 * log_var.detach().cpu()),
                               rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(z.detach().cpu(), ref["z"], rtol=1e-4, atol=1e-5)
    assert tuple(ld) == TERMS
    for k in TERMS:
        assert abs(float(ld[k].detach()) - ref["loss"][k]) <= 1e-4 * abs(ref["loss"][k]), (k, float(ld[k].detach()))
    # the same gradients as the fused plan (the same kernels, the same seeds).  Not asserted bit for
    # bit: the fused plan applies grad_scale inside vae_mmd_fwd, the drop-in path stores dz unscaled
    # and vae_mmd_reseed multiplies it by the device scalar dL/dloss * mmd_coef, and its head / KL
    # seeds are products with dL/dloss too — the same values up to one fp32 rounding per seed element
    # (6e-8), which the backward carries linearly; 1e-6 relative norm allows ~16 such roundings.
    _, runs, _ = run_plan(sd, x, eps, prior, torch.float32, meta["M_N"], **loss_kwargs(meta))
    fused = runs[0][1]
    assert float((g1 - fused).norm() / fused.norm()) <= 1e-6
    # a scaled loss scales every seed, the MMD one included: exactly twice (a power of two)
    _, _, g2 = _step(model, meta, x, eps, prior, scale=2.0)
    assert torch.equal(g2, 2 * g1)
    # a second backward of the same loss (reset_backward) accumulates the same gradient again
    _, _, g3 = _step(model, meta, x, eps, prior, backwards=2)
    assert torch.equal(g3, g1 + g1)


def _formula_tol(z, prior, want, kw):
    """|difference| allowed between two fp32 evaluations of the formula (the device's and the CPU's):
    1e-5 relative per term, plus, for MMD, the fp32 summation error of its three kernel sums — each a
    sum of B(B-1) terms taken to 1e-6 relative (16 ulp) — which the difference S_pp + S_zz - 2 S_pz
    does not shrink; the loss carries that times the MMD coefficient."""
    z, p = z.double().cpu(), prior.double()
    sums = [abs(float(R.compute_kernel(a, b, kw["kernel_type"], kw["latent_var"]).sum()))
            for a, b in ((p, p), (z, z), (p, z), (p, z))]
    B = z.shape[0]
    coef = abs(kw["alpha"] + kw["reg_weight"] - 1.0) / (B * (B - 1))
    extra = {"MMD": 1e-6 * sum(sums), "loss": coef * 1e-6 * sum(sums)}
    return {k: 1e-5 * abs(float(want[k])) + extra.get(k, 0.0) for k in TERMS}


def test_eval_and_foreign_tensors_take_the_torch_formula():
    meta, sd, x, eps, prior, ref = _case()
    model = _model(meta, sd)
    kw = loss_kwargs(meta)
    # foreign tensors (clones of a training forward's outputs): the formula, differentiable
    out = model(x.cuda(), eps=eps.cuda())
    args = [t.detach().clone() for t in out]
    ld = model.loss_function(*args, M_N=meta["M_N"], prior=prior.cuda())
    want = R.info_loss(args[0].cpu(), args[1].cpu(), args[2].cpu(), args[3].cpu(), args[4].cpu(), prior, meta["M_N"], **kw)
    tol = _formula_tol(args[2], prior, want, kw)
    for k in TERMS:
        assert abs(float(ld[k]) - float(want[k])) <= tol[k], (k, float(ld[k]), float(want[k]))
    # eval mode: running-statistics BatchNorm, no autograd, the formula
    model.eval()
    with torch.no_grad():
        out = model(x.cuda(), eps=eps.cuda())
        ld = model.loss_function(*out, M_N=meta["M_N"], prior=prior.cuda())
    assert len(out) == 5 and not out[0].requires_grad
    want = R.info_loss(*[t.cpu() for t in (out[0], out[1], out[2], out[3], out[4])], prior, meta["M_N"], **kw)
    tol = _formula_tol(out[2], prior, want, kw)
    for k in TERMS:
        assert abs(float(ld[k]) - float(want[k])) <= tol[k], (k, float(ld[k]), float(want[k]))
    # without `prior` the model draws one (info_vae.py:220): finite, and different between calls
    a = float(model.loss_function(*out, M_N=meta["M_N"])["MMD"])
    b = float(model.loss_function(*out, M_N=meta["M_N"])["MMD"])
    assert a != b and all(map(lambda v: v == v and abs(v) < 1e6, (a, b)))


def test_reference_keyed_state_dict_round_trip():
    meta, sd, *_ = _case()
    model = _model(meta, sd)
    got = model.state_dict()
    assert list(got) == list(sd)
    for k, v in sd.items():
        assert torch.equal(got[k].cpu(), v), k
    from vae_amd.models import InfoVAE
    other = InfoVAE(3, 128, dtype=torch.float32, device="cuda")
    other.load_state_dict({k: v.clone() for k, v in got.items()}, strict=True)
    assert torch.equal(other.flat.detach(), model.flat.detach())


def test_eval_plan_with_a_fused_info_loss_is_rejected_at_construction():
    """An eval plan builds no MMD call, so a fused VAE_LOSS_INFO ELBO would have no partials to add:
    the combination is an error when the plan is built, not when it runs."""
    from vae_amd.net import StepPlan, VAENet
    net = VAENet(latent_dim=128, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="fused_loss=False"):
        StepPlan(net, 8, loss="info", training=False)
    plan = StepPlan(net, 8, loss="info", training=False, fused_loss=False)
    assert plan.prior is None and not any(fn in ("vae_mmd_fwd", "vae_elbo_fwd") for fn, _ in plan.fwd_calls)
