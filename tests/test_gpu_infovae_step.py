"""The fused InfoVAE step (StepPlan(loss='info'): vae_mmd_fwd behind the reparameterization, the
VAE_LOSS_INFO ELBO, the fused backward) against the reference's golden vectors and the restatement
tests/infovae_ref.py (models/info_vae.py:123-229).

fp32 plan: loss terms (MMD included) within 1e-4 relative of the golden values / the restatement,
gradients within parity_util.grad_bar of the restatement's, a rerun bit-identical.  bf16 plan (the
fused bottleneck route) at B=64 against the fp32 restatement with the restatement under CPU bf16
autocast as yardstick: the bars of tests/test_gpu_bf16_shapes.py.  With the config's parameters
the MMD term is ~all of the encoder's gradient, so a missing or mis-scaled MMD seed fails the
encoder-side gradient checks here.

The bf16 step is not bit-reproducible (fp32 atomics in the bottleneck and the BatchNorm sums, then
bf16 rounding of the activations), and MMD = S_pp + S_zz - 2 S_pz is a difference of sums ~33 times
its size, so its value moves from step to step.  Measured over 400 steps of this very case on an
MI355X (4 plans x 100): MMD 79.5484 .. 79.5719 (3.0e-4 relative between steps), loss 6.92505 ..
6.92562, Reconstruction_Loss 0.467706 .. 0.467720, KLD -16.46778 .. -16.46660; the worst error
against the fp32 restatement was 0.32 (loss), 0.55 (Reconstruction_Loss), 0.15 (MMD), 0.02 (KLD) of
its `_loss_bar`, the worst gradient (decoder.2.1.weight) 0.65 of its `_grad_bar`.  So every quantity
compared in the bf16 test is taken from ONE step (run_plan keeps each step's own mu | log_var):
two different steps' MMD can differ by more than the 1e-4 of the own-inputs check."""
import functools

import pytest
import torch

import infovae_ref as R
from infovae_golden import CASES, TERMS, case_inputs, load_case, loss_kwargs
from parity_util import grad_bar
from test_gpu_bf16_shapes import _grad_bar, _loss_bar, _pre_bn_bias

pytestmark = pytest.mark.gpu

YAML = dict(alpha=-9.0, beta=10.5, reg_weight=110, kernel_type="imq", latent_var=2.0)   # configs/vae/infovae.yaml
M_N = 2.5e-4


def run_plan(sd, x, eps, prior, dtype, M_N, **kw):
    from vae_amd import _lib as L
    from vae_amd.net import StepPlan, VAENet
    net = VAENet(latent_dim=eps.shape[1], dtype=dtype, device="cuda")
    net.load_reference_state_dict(sd)
    plan = StepPlan(net, x.shape[0], loss="info", kld_weight=M_N, **kw)
    plan.x.copy_(x)
    plan.eps.copy_(eps)
    plan.prior.copy_(prior)
    st = L.stream_ptr()
    runs = []
    for _ in range(2):
        L.call("vae_step_begin", plan.zero.data_ptr(), plan.zero.numel() * 4, plan.step.data_ptr(), st)
        plan.forward(st)
        plan.backward(st)
        torch.cuda.synchronize()
        runs.append((plan.loss_dict(), plan.grads.clone(), plan.dz_mmd.clone(), plan.mulv.clone()))
    grads = {k: v.cpu() for k, v in net.layout.export_reference(runs[0][1]).items()}
    return plan, runs, grads


@functools.lru_cache(maxsize=None)
def _b64():
    from oracle import vae_oracle as O
    sd = O.make_params(O.vanilla_param_spec(), 1265)
    x, eps = O.make_inputs(64, 128, 31)
    return sd, x, eps, R.make_prior(64, 128, 31)


def _check_fp32(sd, x, eps, prior, M_N, kw, want_terms=None):
    ref, spread = R.with_spread(sd, x, eps, prior, M_N=M_N, **kw)
    plan, runs, grads = run_plan(sd, x, eps, prior, torch.float32, M_N, **kw)
    assert not plan.latent_fused
    got = runs[0][0]
    assert tuple(got) == TERMS
    for src in (ref["loss"], want_terms or ref["loss"]):
        for k in TERMS:
            print(f"{k}: hip {got[k]:.8g} want {src[k]:.8g}")
            assert abs(got[k] - src[k]) <= 1e-4 * abs(src[k]), (k, got[k], src[k])
    worst = 0.0
    for name, gr in ref["grads"].items():
        if _pre_bn_bias(name):
            continue                                    # analytically zero under train-mode BatchNorm
        err = float((grads[name].double() - gr.double()).norm() / gr.double().norm())
        worst = max(worst, err)
        assert err < grad_bar(name, spread), (name, err, grad_bar(name, spread))
    print(f"InfoVAE fp32 B={x.shape[0]} {kw['kernel_type']}: worst gradient rel-norm {worst:.2e}")
    # the same step again: every reduction is ordered
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


@pytest.mark.parametrize("case", CASES)
def test_fp32_step_matches_golden_and_restatement(case):
    meta, _ = load_case(case)
    sd, x, eps, prior = case_inputs(meta)
    _check_fp32(sd, x, eps, prior, meta["M_N"], loss_kwargs(meta), want_terms=meta["loss"])


def test_fp32_step_b64_matches_restatement():
    _check_fp32(*_b64(), M_N, dict(YAML))


def test_bf16_step_b64_tracks_autocast_restatement():
    sd, x, eps, prior = _b64()
    plan, runs, g16 = run_plan(sd, x, eps, prior, torch.bfloat16, M_N, **YAML)
    assert plan.latent_fused                            # the fused bottleneck route
    o32 = R.train_step(sd, x, eps, prior, M_N=M_N, **YAML)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        oac = R.train_step(sd, x, eps, prior, M_N=M_N, **YAML)
    got = runs[0][0]
    for k in TERMS:
        ref = o32["loss"][k]
        print(f"{k}: hip {got[k]:.8g} fp32 {ref:.8g} autocast {oac['loss'][k]:.8g}; rel err hip "
              f"{abs(got[k] - ref) / abs(ref):.2e} bar {2 * abs(oac['loss'][k] - ref) / abs(ref) + 1e-4:.2e}")
    _loss_bar([got[k] for k in TERMS], o32, oac, TERMS)
    assert _grad_bar(g16, o32, oac, "InfoVAE B=64 bf16", _pre_bn_bias) >= 30
    # The MMD term is computed from fp32 mu | log_var (never the bf16 z): the kernel's value against
    # the formula in fp64 on the fp32 reparameterization of THE SAME step's mu | log_var (runs[0]'s
    # own copy: the step is not bit-reproducible, see the module docstring), with the eps and prior
    # this test wrote.  It shows that on the fused-latent route the kernel read this step's eps and
    # prior and a mu | log_var equal to the plan's at the op's own 1e-4 bar.  It does NOT show that
    # plan.mulv is the right mu | log_var: that buffer is on both sides.  A wrong or stale mu | log_var
    # is left to the autocast bars above (a zero or previous-step buffer moves MMD by far more than
    # they allow: z = eps alone gives MMD ~ 0 against 79.6).
    mulv = runs[0][3].cpu()
    z = mulv[:, :128] + eps * torch.exp(0.5 * mulv[:, 128:])
    m = float(R.compute_mmd(z.double(), prior.double(), "imq", 2.0))
    print(f"MMD on the step's own mu|log_var: hip {got['MMD']:.8g} fp64 {m:.8g}; rel err {abs(got['MMD'] - m) / abs(m):.2e}")
    assert abs(got["MMD"] - m) <= 1e-4 * abs(m), (got["MMD"], m)
