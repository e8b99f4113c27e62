"""The fused MIWAE step (StepPlan(loss='miwae', samples=K, estimates=M): the decoder at B*M*K rows, the
VAE_LOSS_MIWAE ELBO, the fused backward) against the reference's golden vectors and the restatement
tests/miwae_ref.py (models/miwae.py:124-164).

fp32 plan: the three loss terms within 1e-4 relative of the golden values / the restatement, gradients
within parity_util.grad_bar of the restatement's, a rerun bit-identical; the golden cases (B, M, K) =
(4,3,5) and (2,5,5), and the restatement at (1,2,3) (one image) and (7,2,3) (42 rows: a partial tile).
bf16 plan (the fused bottleneck route) at (16,3,5) — 240 rows — and (13,3,5) — a partial last batch,
195 rows — against the fp32 restatement with the restatement under CPU bf16 autocast as yardstick: the
bars of tests/test_gpu_bf16_shapes.py, every compared quantity from one step.

That the weighting is inside the groups of K, not over an image's M*K rows, is pinned on crafted
inputs by tests/test_gpu_miwae.py: a step's own log-weights at initialisation are too close together
to tell the groupings apart."""
import functools

import pytest
import torch

import miwae_ref as R
from golden_util import load_case
from parity_util import grad_bar
from test_gpu_bf16_shapes import _grad_bar, _loss_bar, _pre_bn_bias

pytestmark = pytest.mark.gpu

M_N = 2.5e-4


def run_plan(sd, x, eps, dtype, M_N, M, K, **kw):
    from vae_amd import _lib as L
    from vae_amd.net import StepPlan, VAENet
    net = VAENet(latent_dim=eps.shape[-1], dtype=dtype, device="cuda")
    net.load_reference_state_dict(sd)
    plan = StepPlan(net, x.shape[0], loss="miwae", samples=K, estimates=M, kld_weight=M_N, **kw)
    assert plan.S == M * K and plan.recon.shape[0] == x.shape[0] * M * K
    plan.x.copy_(x)
    plan.eps.copy_(eps.reshape(plan.eps.shape))
    st = L.stream_ptr()
    runs = []
    for _ in range(2):
        L.call("vae_step_begin", plan.zero.data_ptr(), plan.zero.numel() * 4, plan.step.data_ptr(), st)
        plan.forward(st)
        plan.backward(st)
        torch.cuda.synchronize()
        runs.append((plan.loss_dict(), plan.grads.clone(), plan.per_img.clone(), plan.head_coef.clone()))
    grads = {k: v.cpu() for k, v in net.layout.export_reference(runs[0][1]).items()}
    return plan, runs, grads


@functools.lru_cache(maxsize=None)
def _inputs(B, S, seed):
    from oracle import vae_oracle as O
    sd = O.make_params(O.vanilla_param_spec(), 1265)
    x, eps = O.make_inputs(B, 128, seed, samples=S)
    return sd, x, eps


def _check_fp32(sd, x, eps, M_N, M, K, want_terms=None):
    ref, spread = R.with_spread(sd, x, eps, M_N=M_N, M=M, K=K)
    plan, runs, grads = run_plan(sd, x, eps, torch.float32, M_N, M, K)
    assert not plan.latent_fused and not plan.elbo_in_head and not plan.wide_head
    got = runs[0][0]
    assert tuple(got) == R.TERMS
    for src in (ref["loss"], want_terms or ref["loss"]):
        for k in R.TERMS:
            print(f"{k}: hip {got[k]:.8g} want {src[k]:.8g}")
            assert abs(got[k] - src[k]) <= 1e-4 * abs(src[k]), (k, got[k], src[k])
    per = runs[0][2].cpu()
    assert float((per - ref["per_row_mse"]).norm() / ref["per_row_mse"].norm()) <= 1e-4
    worst = 0.0
    for name, gr in ref["grads"].items():
        if _pre_bn_bias(name):
            continue                                    # analytically zero under train-mode BatchNorm
        err = float((grads[name].double() - gr.double()).norm() / gr.double().norm())
        worst = max(worst, err)
        assert err < grad_bar(name, spread), (name, err, grad_bar(name, spread))
    print(f"MIWAE fp32 (B,M,K)=({x.shape[0]},{M},{K}): worst gradient rel-norm {worst:.2e}")
    # the same step again: every reduction is ordered
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:]))
    return ref


@pytest.mark.parametrize("case", R.CASES)
def test_fp32_step_matches_golden_and_restatement(case):
    meta, _ = load_case(case)
    sd, x, eps = R.case_inputs(meta)
    M, K = R.case_mk(meta)
    _check_fp32(sd, x, eps, meta["M_N"], M, K, want_terms=meta["loss"])


@pytest.mark.parametrize("B,M,K", [(1, 2, 3), (7, 2, 3)])
def test_fp32_step_small_shapes_match_restatement(B, M, K):
    _check_fp32(*_inputs(B, M * K, 40 + B), M_N, M, K)


@pytest.mark.parametrize("B,M,K", [(16, 3, 5), (13, 3, 5)])
def test_bf16_step_tracks_autocast_restatement(B, M, K):
    sd, x, eps = _inputs(B, M * K, 31)
    plan, runs, g16 = run_plan(sd, x, eps, torch.bfloat16, M_N, M, K)
    assert plan.latent_fused                            # the fused bottleneck route
    o32 = R.train_step(sd, x, eps, M_N=M_N, M=M, K=K)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        oac = R.train_step(sd, x, eps, M_N=M_N, M=M, K=K)
    got = runs[0][0]
    for k in R.TERMS:
        ref = o32["loss"][k]
        print(f"{k}: hip {got[k]:.8g} fp32 {ref:.8g} autocast {oac['loss'][k]:.8g}; rel err hip "
              f"{abs(got[k] - ref) / abs(ref):.2e} bar {2 * abs(oac['loss'][k] - ref) / abs(ref) + 1e-4:.2e}")
    _loss_bar([got[k] for k in R.TERMS], o32, oac, R.TERMS)
    assert _grad_bar(g16, o32, oac, f"MIWAE ({B},{M},{K}) bf16", _pre_bn_bias) >= 30
