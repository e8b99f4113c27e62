"""The fused LogCoshVAE step (StepPlan(loss='logcosh'): vae_logcosh_loss closing the forward, its
dL/drecon seeding the head backward and its kl_coef the bottleneck backward) against the reference's
golden vectors and the restatement tests/logcosh_ref.py (models/logcosh_vae.py:120-155).

fp32 graph step against both golden cases at the bars of
test_gpu_recon_loss.py::test_fused_graph_step_with_recon_loss_matches_reference (loss terms 1e-4,
recon_head atol 1e-4, gradient norms 1e-3, BatchNorm affine 3e-3); B = 1, 7 and 19 against the
restatement with parity_util.grad_bar; a bf16 plan at B = 8 on both bottleneck routes: the loss terms
recomputed in fp64 from the plan's own recon / mulv buffers, the routes' fc_mu | fc_var gradients at
the autocast bar of tests/test_gpu_routes.py, and the KL seed shown to arrive."""
import functools

import numpy as np
import pytest
import torch

import logcosh_ref as R
from golden_util import load_case, summary
from parity_util import grad_bar

pytestmark = pytest.mark.gpu

YAML = dict(alpha=10.0, beta=1.0)                       # configs/vae/logcosh_vae.yaml
M_N = 0.00025


def _model(sd, dtype, **kw):
    from vae_amd.models import vae_models
    m = vae_models["LogCoshVAE"](in_channels=3, latent_dim=128, **kw, dtype=dtype, device="cuda")
    m.load_reference_state_dict(sd)
    return m.train()


@pytest.mark.parametrize("case", R.CASES)
def test_fused_graph_step_matches_reference(case):
    meta, ref = load_case(case)
    sd, x, eps = R.case_inputs(meta)
    model = _model(sd, torch.float32, **R.loss_kwargs(meta))
    step = model.fused_train_step(x.shape[0], meta["M_N"], lr=meta["lr"], graph=True)
    fns = [fn for fn, _ in step.plan.fwd_calls]
    assert "vae_logcosh_loss" in fns and "vae_elbo_fwd" not in fns and "vae_recon_loss" not in fns
    assert step.plan.seed_recon and not step.plan.elbo_in_head
    step(x.cuda(), eps.cuda())
    torch.cuda.synchronize()
    got = step.loss_terms()
    assert step.plan.loss_names == R.TERMS and tuple(step.plan.loss_dict()) == R.TERMS
    for i, k in enumerate(R.TERMS):
        v = meta["loss"][k]
        print(f"{case} {k}: hip {got[i]:.8g} reference {v:.8g}")
        assert abs(got[i] - v) <= 1e-4 * abs(v), (k, got[i], v)
    n_head = ref["recon_head"].shape[0]
    np.testing.assert_allclose(step.plan.recon[:n_head].cpu().numpy(), ref["recon_head"], rtol=0, atol=1e-4)
    g_all = model.net.layout.export_reference(step.plan.grads)
    checked = 0
    for name in meta["param_names"]:
        if R.pre_bn_bias(name):
            continue
        rs, st = ref[f"grad_stats/{name}"], summary(g_all[name])
        bound = 3e-3 if name.endswith(".1.weight") or name.endswith(".1.bias") else 1e-3
        assert abs(st[1] - rs[1]) / max(rs[1], 1e-12) < bound, (name, st, rs)
        checked += 1
    assert checked >= 20
    # per-image MSE of the step (experiment.py:60-62) from the head's SSE, whatever the model's loss is
    per = step.plan.per_img.cpu()
    want = ((step.plan.recon.cpu() - x) ** 2).mean(dim=[1, 2, 3])
    torch.testing.assert_close(per, want, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(per.numpy(), ref["per_img_mse"], rtol=1e-3)


def test_eval_plan_has_no_loss_call():
    from vae_amd.net import StepPlan, VAENet
    net = VAENet(latent_dim=128, dtype=torch.float32, device="cuda")
    plan = StepPlan(net, 8, loss="logcosh", training=False, **YAML)
    fns = [fn for fn, _ in plan.fwd_calls]
    assert not any(fn in ("vae_logcosh_loss", "vae_elbo_fwd", "vae_recon_loss") for fn in fns)
    with pytest.raises(ValueError, match="alpha"):
        StepPlan(net, 8, loss="logcosh")                # alpha's default is InfoVAE's -0.5


def _run_plan(sd, x, eps, dtype, kld_weight=M_N, hidden_dims=None, **kw):
    from vae_amd import _lib as L
    from vae_amd.net import StepPlan, VAENet
    net = VAENet(latent_dim=eps.shape[1], hidden_dims=hidden_dims, dtype=dtype, device="cuda")
    net.load_reference_state_dict(sd)
    plan = StepPlan(net, x.shape[0], loss="logcosh", kld_weight=kld_weight, **{**YAML, **kw})
    plan.x.copy_(x)
    plan.eps.copy_(eps)
    st = L.stream_ptr()
    runs = []
    for _ in range(2):
        L.call("vae_step_begin", plan.zero.data_ptr(), plan.zero.numel() * 4, plan.step.data_ptr(), st)
        plan.forward(st)
        plan.backward(st)
        torch.cuda.synchronize()
        runs.append((plan.loss_dict(), plan.grads.clone()))
    grads = {k: v.cpu() for k, v in net.layout.export_reference(runs[0][1]).items()}
    return plan, runs, grads


@functools.lru_cache(maxsize=None)
def _inputs(B, seed):
    from oracle import vae_oracle as O
    sd = O.make_params(O.vanilla_param_spec(), 1265)
    x, eps = O.make_inputs(B, 128, seed)
    return sd, x, eps


def _check_fp32(sd, x, eps, hidden_dims=None):
    B = x.shape[0]
    ref, spread = R.with_spread(sd, x, eps, M_N=M_N, hidden_dims=hidden_dims, **YAML)
    plan, runs, grads = _run_plan(sd, x, eps, torch.float32, hidden_dims=hidden_dims)
    assert not plan.latent_fused and plan.wide_head == (hidden_dims is not None)
    got = runs[0][0]
    for k in R.TERMS:
        print(f"B={B} {k}: hip {got[k]:.8g} want {ref['loss'][k]:.8g}")
        assert abs(got[k] - ref["loss"][k]) <= 1e-4 * abs(ref["loss"][k]), (k, got[k], ref["loss"][k])
    worst = 0.0
    for name, gr in ref["grads"].items():
        if R.pre_bn_bias(name):
            continue                                    # analytically zero under train-mode BatchNorm
        err = float((grads[name].double() - gr.double()).norm() / gr.double().norm())
        worst = max(worst, err)
        assert err < grad_bar(name, spread), (name, err, grad_bar(name, spread))
    print(f"LogCoshVAE fp32 B={B}: worst gradient rel-norm {worst:.2e}")
    # the same step again: every reduction is ordered
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    return plan


@pytest.mark.parametrize("B", [1, 7, 19])
def test_fp32_step_last_batch_sizes_match_restatement(B):
    _check_fp32(*_inputs(B, 60 + B))


def test_fp32_wide_head_step_matches_restatement():
    """A first layer wider than 32 channels takes the conv-GEMM head: its seed is vae_recon_bwd's, from
    the grad_recon the loss kernel wrote (no mean-MSE seed from vae_recon_fwd)."""
    from oracle import vae_oracle as O
    hd = [64, 128, 256, 256, 512]
    sd = O.make_params(O.vanilla_param_spec(hidden_dims=hd), 1265)
    x, eps = O.make_inputs(4, 128, 77)
    plan = _check_fp32(sd, x, eps, hidden_dims=hd)
    assert "vae_recon_bwd" in [fn for fn, _ in plan.bwd_calls]
    with pytest.raises(ValueError, match="vae_logcosh_loss"):
        plan.run_elbo(0, "logcosh", M_N)


def test_bf16_step_both_bottleneck_routes():
    B = 8
    sd, x, eps = _inputs(B, 31)
    o32 = R.train_step(sd, x, eps, M_N=M_N, **YAML)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        oac = R.train_step(sd, x, eps, M_N=M_N, **YAML)
    grads = {}
    for fused in (True, False):
        plan, runs, g16 = _run_plan(sd, x, eps, torch.bfloat16, latent_kernels=fused)
        assert plan.latent_fused == fused
        fns = [fn for fn, _ in plan.bwd_calls]
        assert ("vae_latent_dec_bwd" in fns) == fused
        # the loss terms from the plan's own buffers, in fp64
        rl, kld, loss, seed = R.terms64(plan.recon.cpu(), x, plan.mulv.cpu(), YAML["alpha"], YAML["beta"] * M_N)
        got = runs[-1][0]          # (the buffers hold the last run's values; bf16 runs differ by their atomics)
        print(f"latent_kernels={fused}: {got} fp64 {loss:.9g} {rl:.9g} {-kld:.9g}")
        for k, want in zip(R.TERMS, (loss, rl, -kld)):
            assert abs(got[k] - want) <= 1e-5 * abs(want), (fused, k, got[k], want)
        assert float((plan.grad_recon.cpu().double() - seed).norm() / seed.norm()) < 1e-5
        assert bool((plan.kl_coef.cpu() == np.float32(YAML["beta"] * M_N) / np.float32(B)).all())
        grads[fused] = g16
        # each route's fc_mu | fc_var gradients at the bar tests/test_gpu_routes.py holds a route to:
        # within twice the bf16-autocast restatement's own error + 2e-3 of the fp32 restatement
        for name in ("fc_mu.weight", "fc_mu.bias", "fc_var.weight", "fc_var.bias"):
            d = o32["grads"][name].double()
            e_ac = float((oac["grads"][name].double() - d).norm() / d.norm())
            e_hip = float((g16[name].double() - d).norm() / d.norm())
            print(f"latent_kernels={fused} {name}: hip {e_hip:.3e} autocast {e_ac:.3e}")
            assert e_hip <= 2 * e_ac + 2e-3, (fused, name, e_hip, e_ac)
    # the KL seed really arrives: without it (kld_weight = 0) fc_var's gradient is another one.  In the
    # restatement the KL term is this share of it:
    none = R.train_step(sd, x, eps, M_N=0.0, **YAML)
    a, b = o32["grads"]["fc_var.weight"].double(), none["grads"]["fc_var.weight"].double()
    share = float((a - b).norm() / a.norm())
    for fused in (True, False):
        plan, runs, g0 = _run_plan(sd, x, eps, torch.bfloat16, kld_weight=0.0, latent_kernels=fused)
        assert bool((plan.kl_coef == 0).all())
        a, b = grads[fused]["fc_var.weight"].double(), g0["fc_var.weight"].double()
        moved = float((a - b).norm() / a.norm())
        print(f"latent_kernels={fused}: fc_var.weight moves by {moved:.3e} without the KL seed (restatement {share:.3e})")
        assert moved > 0.5 * share > 0.0
