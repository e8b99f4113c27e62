"""The fused DIP-VAE step (StepPlan(loss='dip'): vae_dip_fwd as soon as mu | log_var are final, the
VAE_LOSS_DIP ELBO, the fused backward) against the reference's golden vectors and the restatement
tests/dipvae_ref.py (models/dip_vae.py:120-164).

fp32 plan: all four loss terms within 1e-4 relative of the golden values / the restatement, gradients
within parity_util.grad_bar of the restatement's, a rerun bit-identical; B = 16 and 8 (the golden
cases), 1 (a one-row Gram matrix; experiment.test_step's batch) and 7 (fewer rows than a k-step of
the batch product holds).  bf16 plan (the fused bottleneck route) at B = 64 against the fp32
restatement with the restatement under CPU bf16 autocast as yardstick: the bars of
tests/test_gpu_bf16_shapes.py, every compared quantity from one step.

With the config's lambdas the DIP term is nearly all of fc_mu's gradient (asserted on the
restatement below), so a missing or wrong DIP seed fails the encoder-side gradient checks here."""
import functools

import pytest
import torch

import dipvae_ref as R
from golden_util import load_case
from parity_util import grad_bar
from test_gpu_bf16_shapes import _grad_bar, _loss_bar, _pre_bn_bias

pytestmark = pytest.mark.gpu

YAML = dict(lambda_diag=0.05, lambda_offdiag=0.1)        # configs/vae/dip_vae.yaml
M_N = 1.0


def run_plan(sd, x, eps, dtype, M_N, hidden_dims=None, **kw):
    from vae_amd import _lib as L
    from vae_amd.net import StepPlan, VAENet
    net = VAENet(latent_dim=eps.shape[1], hidden_dims=hidden_dims, dtype=dtype, device="cuda")
    net.load_reference_state_dict(sd)
    plan = StepPlan(net, x.shape[0], loss="dip", kld_weight=M_N, **kw)
    plan.x.copy_(x)
    plan.eps.copy_(eps)
    st = L.stream_ptr()
    runs = []
    for _ in range(2):
        L.call("vae_step_begin", plan.zero.data_ptr(), plan.zero.numel() * 4, plan.step.data_ptr(), st)
        plan.forward(st)
        plan.backward(st)
        torch.cuda.synchronize()
        runs.append((plan.loss_dict(), plan.grads.clone(), plan.dmulv_dip.clone(), plan.mulv.clone()))
    grads = {k: v.cpu() for k, v in net.layout.export_reference(runs[0][1]).items()}
    return plan, runs, grads


@functools.lru_cache(maxsize=None)
def _inputs(B, seed):
    from oracle import vae_oracle as O
    sd = O.make_params(O.vanilla_param_spec(), 1265)
    x, eps = O.make_inputs(B, 128, seed)
    return sd, x, eps


def _check_fp32(sd, x, eps, M_N, kw, want_terms=None, hidden_dims=None):
    ref, spread = R.with_spread(sd, x, eps, M_N=M_N, hidden_dims=hidden_dims, **kw)
    plan, runs, grads = run_plan(sd, x, eps, torch.float32, M_N, hidden_dims=hidden_dims, **kw)
    assert not plan.latent_fused and plan.wide_head == (hidden_dims is not None)
    got = runs[0][0]
    assert tuple(got) == R.TERMS
    for src in (ref["loss"], want_terms or ref["loss"]):
        for k in R.TERMS:
            print(f"{k}: hip {got[k]:.8g} want {src[k]:.8g}")
            assert abs(got[k] - src[k]) <= 1e-4 * abs(src[k]), (k, got[k], src[k])
    worst = 0.0
    for name, gr in ref["grads"].items():
        if _pre_bn_bias(name):
            continue                                    # analytically zero under train-mode BatchNorm
        err = float((grads[name].double() - gr.double()).norm() / gr.double().norm())
        worst = max(worst, err)
        assert err < grad_bar(name, spread), (name, err, grad_bar(name, spread))
    print(f"DIP-VAE fp32 B={x.shape[0]} {kw}: worst gradient rel-norm {worst:.2e}")
    # the same step again: every reduction is ordered
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    return ref


@pytest.mark.parametrize("case", R.CASES)
def test_fp32_step_matches_golden_and_restatement(case):
    meta, _ = load_case(case)
    sd, x, eps = R.case_inputs(meta)
    _check_fp32(sd, x, eps, meta["M_N"], R.loss_kwargs(meta), want_terms=meta["loss"])


@pytest.mark.parametrize("B", [1, 7])
def test_fp32_step_small_batches_match_restatement(B):
    _check_fp32(*_inputs(B, 40 + B), M_N, dict(YAML))


def test_fp32_wide_head_step_matches_restatement():
    """A first layer wider than 32 channels takes the conv-GEMM head, whose reconstruction seed is
    written by vae_recon_fwd: for DIP-VAE the seed of the SUM, not of the mean."""
    from oracle import vae_oracle as O
    hd = [64, 128, 256, 256, 512]
    sd = O.make_params(O.vanilla_param_spec(hidden_dims=hd), 1265)
    x, eps = O.make_inputs(4, 128, 77)
    _check_fp32(sd, x, eps, M_N, dict(YAML), hidden_dims=hd)


def test_dip_term_dominates_the_fc_mu_gradient_in_the_restatement():
    """So the gradient checks above cannot pass with the DIP seed missing: without the term fc_mu's
    gradient moves by most of its norm (B = 16, the yaml's lambdas)."""
    meta, _ = load_case("dipvae_b16")
    sd, x, eps = R.case_inputs(meta)
    full = R.train_step(sd, x, eps, M_N=meta["M_N"], **R.loss_kwargs(meta))
    none = R.train_step(sd, x, eps, M_N=meta["M_N"], lambda_diag=0.0, lambda_offdiag=0.0)
    a, b = full["grads"]["fc_mu.weight"].double(), none["grads"]["fc_mu.weight"].double()
    assert float((a - b).norm() / a.norm()) > 0.5


def test_bf16_step_b64_tracks_autocast_restatement():
    sd, x, eps = _inputs(64, 31)
    plan, runs, g16 = run_plan(sd, x, eps, torch.bfloat16, M_N, **YAML)
    assert plan.latent_fused                            # the fused bottleneck route
    o32 = R.train_step(sd, x, eps, M_N=M_N, **YAML)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        oac = R.train_step(sd, x, eps, M_N=M_N, **YAML)
    got = runs[0][0]
    for k in R.TERMS:
        ref = o32["loss"][k]
        print(f"{k}: hip {got[k]:.8g} fp32 {ref:.8g} autocast {oac['loss'][k]:.8g}; rel err hip "
              f"{abs(got[k] - ref) / abs(ref):.2e} bar {2 * abs(oac['loss'][k] - ref) / abs(ref) + 1e-4:.2e}")
    _loss_bar([got[k] for k in R.TERMS], o32, oac, R.TERMS)
    assert _grad_bar(g16, o32, oac, "DIP-VAE B=64 bf16", _pre_bn_bias) >= 30
    # The DIP term is computed from the step's own fp32 mu | log_var: the kernel's value and gradient
    # against fp64 on runs[0]'s own copy of that buffer, at the op's own 1e-4 bars.  (That plan.mulv is
    # the right mu | log_var is left to the autocast bars above: the buffer is on both sides here.)
    mulv = runs[0][3].cpu()
    d, gm, gl = R.dip_grad64(mulv[:, :128], mulv[:, 128:], **YAML)
    print(f"DIP_Loss on the step's own mu|log_var: hip {got['DIP_Loss']:.8g} fp64 {d:.8g}")
    assert abs(got["DIP_Loss"] - d) <= 1e-4 * abs(d), (got["DIP_Loss"], d)
    seed = runs[0][2].cpu().double()
    assert float((seed[:, :128] - gm).norm() / gm.norm()) <= 1e-4
    assert float((seed[:, 128:] - gl).norm() / gl.norm()) <= 1e-4
