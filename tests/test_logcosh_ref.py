"""Pin the LogCoshVAE restatement (tests/logcosh_ref.py) against the reference's golden vectors, and
the stable form of its reconstruction term against the reference's literal expression (both sides
ATen on the CPU)."""
import math

import numpy as np
import pytest
import torch

import logcosh_ref as R
from golden_util import load_case, rel_err, summary
from oracle import vae_oracle as O


@pytest.mark.parametrize("case", R.CASES)
def test_restatement_matches_reference(case):
    meta, ref = load_case(case)
    sd, x, eps = R.case_inputs(meta)
    out = R.train_step(sd, x, eps, M_N=meta["M_N"], **R.loss_kwargs(meta))
    assert tuple(out["loss"]) == tuple(meta["loss"]) == R.TERMS
    for k, v in meta["loss"].items():
        assert math.isfinite(v)
        assert abs(out["loss"][k] - v) <= 1e-6 * abs(v), (k, out["loss"][k], v)
    recon = out["recon"]
    n_head = ref["recon_head"].shape[0]
    assert rel_err(recon[:n_head].numpy(), ref["recon_head"]) < 1e-5
    np.testing.assert_allclose(recon.reshape(recon.shape[0], -1).double().sum(1).numpy(), ref["recon_sum"],
                               rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(out["per_img_mse"].numpy(), ref["per_img_mse"], rtol=1e-5)
    for k in ("mu", "log_var"):
        assert rel_err(out[k].numpy(), ref[k]) < 1e-5, k
    for name in meta["param_names"]:
        if R.pre_bn_bias(name):
            continue            # analytically zero: what either side computes is rounding noise
        g = out["grads"][name]
        st, ref_st = summary(g), ref[f"grad_stats/{name}"]
        assert abs(st[1] - ref_st[1]) <= 1e-4 * max(ref_st[1], 1e-12) + 1e-12, (name, st, ref_st)
        np.testing.assert_allclose(g.flatten()[:64].numpy(), ref[f"grad_head/{name}"], rtol=1e-3,
                                   atol=1e-4 * ref_st[2] + 1e-12)
        p = sd[name].clone()
        O.adam_step(p, g, p.new_zeros(p.shape), p.new_zeros(p.shape), 1, meta["lr"])
        np.testing.assert_allclose(p.flatten()[:64].numpy(), ref[f"new_head/{name}"], rtol=1e-5, atol=1e-6)
    for k, v in out["running"].items():
        np.testing.assert_allclose(v.numpy(), ref[f"running/{k}"], rtol=1e-5, atol=1e-6)


def _residual(case):
    """t = recon - x of a golden case's forward (fp32, from the restatement)."""
    meta, _ = load_case(case)
    sd, x, eps = R.case_inputs(meta)
    P = {k: v.detach().clone() for k, v in sd.items()}
    with torch.no_grad():
        mu, lv = O.vanilla_encode(P, x, list(O.DEFAULT_HIDDEN), True, {})
        recon = O.vanilla_decode(P, O.reparameterize(mu, lv, eps), list(O.DEFAULT_HIDDEN), True, {})
    return meta, recon - x


@pytest.mark.parametrize("case", R.CASES)
def test_literal_and_stable_forms_agree_in_fp64(case):
    """The same function: in fp64 (where exp(-2*alpha*t) is far from overflowing) the two forms agree to
    rounding, value and gradient, on the golden inputs — and the gradient is tanh(alpha*t)/N."""
    meta, t = _residual(case)
    alpha = R.loss_kwargs(meta)["alpha"]
    t64 = t.double().requires_grad_(True)
    lit, stab = R.recon_literal(t64, alpha), R.recon_stable(t64, alpha)
    # the literal form's log 2 is torch.log(torch.tensor(2.0)), an fp32 value whatever t's dtype is:
    # the forms differ by exactly (fp32 log 2 - log 2) / alpha = 1.9e-9 / alpha, and by rounding
    ln2_gap = (float(torch.log(torch.tensor(2.0))) - math.log(2.0)) / alpha
    assert abs(float(lit.detach()) - float(stab.detach()) + ln2_gap) <= 1e-13 * abs(float(lit.detach()))
    (gl,), (gs,) = torch.autograd.grad(lit, t64), torch.autograd.grad(stab, t64)
    want = torch.tanh(alpha * t64.detach()) / t64.numel()
    assert float((gl - want).norm() / want.norm()) < 1e-13
    assert float((gs - want).norm() / want.norm()) < 1e-13
    # and the fp32 literal form is the fixture's Reconstruction_Loss, the stable one within fp32 rounding
    assert float(R.recon_literal(t, alpha)) == pytest.approx(meta["loss"]["Reconstruction_Loss"], rel=1e-6)
    assert float(R.recon_stable(t, alpha)) == pytest.approx(float(stab.detach()), rel=1e-6)


def test_literal_form_overflows_at_the_constructor_default():
    """The reason for the documented deviation: at alpha = 100 the reference's fp32 expression is inf on
    the b8 inputs (t < -0.44 occurs) and its gradient NaN, while the stable form is finite and equals
    fp64."""
    _, t = _residual("logcosh_b8")
    assert float(t.min()) < -0.44
    t32 = t.clone().requires_grad_(True)
    lit = R.recon_literal(t32, 100.0)
    assert math.isinf(float(lit.detach()))
    (g,) = torch.autograd.grad(lit, t32)
    assert bool(torch.isnan(g).any())
    t32 = t.clone().requires_grad_(True)
    stab = R.recon_stable(t32, 100.0)
    (g,) = torch.autograd.grad(stab, t32)
    stab = stab.detach()
    assert math.isfinite(float(stab)) and bool(torch.isfinite(g).all())
    want = float(R.recon_stable(t.double(), 100.0))
    print("stable fp32", float(stab), "fp64", want)
    assert float(stab) == pytest.approx(want, rel=1e-6)
    assert want == pytest.approx(0.5723239, rel=1e-6)
