"""Pin the DIP-VAE restatement (tests/dipvae_ref.py) against the reference's golden vectors, at the
bars tests/test_oracle_golden.py uses for the other models (both sides fp32 ATen on the CPU)."""
import numpy as np
import pytest
import torch

import dipvae_ref as R
from golden_util import load_case, rel_err, summary
from oracle import vae_oracle as O


@pytest.mark.parametrize("case", R.CASES)
def test_restatement_matches_reference(case):
    meta, ref = load_case(case)
    sd, x, eps = R.case_inputs(meta)
    out = R.train_step(sd, x, eps, M_N=meta["M_N"], **R.loss_kwargs(meta))
    assert tuple(out["loss"]) == tuple(meta["loss"]) == R.TERMS
    for k, v in meta["loss"].items():
        assert abs(out["loss"][k] - v) <= 1e-5 * max(abs(v), 1e-3), (k, out["loss"][k], v)
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
            # analytically zero; what either side computes is the rounding noise of a gradient whose
            # scale is the SUM-reduced loss's (1e5 here), in another summation order
            continue
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


@pytest.mark.parametrize("B,D", [(1, 32), (7, 32), (40, 32), (64, 128)])
def test_closed_form_gradient_is_autograd(B, D):
    """The gradient the kernel implements (include/vaehip.h vae_dip_args) against fp64 autograd of the
    restatement: G = d dip/d cov_z, X = 2 c G, d mu = X - mean_d X, d log_var on the diagonal only."""
    g = torch.Generator().manual_seed(B * 1000 + D)
    mu = (0.5 * torch.randn(B, D, generator=g)).double()
    lv = (0.3 * torch.randn(B, D, generator=g)).double()
    ld, lo = 0.05, 0.1
    _, gm, gl = R.dip_grad64(mu, lv, ld, lo)
    c = mu - mu.mean(1, keepdim=True)
    n = min(B, D)
    idx = torch.arange(n)
    cov_z = c.t() @ c + (2 * lv[idx, idx]).exp().mean()
    G = 2 * lo * cov_z
    G[torch.arange(D), torch.arange(D)] = 2 * ld * (torch.diagonal(cov_z) - 1)
    X = 2 * c @ G
    want_m = X - X.mean(1, keepdim=True)
    want_l = torch.zeros_like(lv)
    want_l[idx, idx] = G.sum() * 2 * (2 * lv[idx, idx]).exp() / n
    assert float((gm - want_m).norm() / gm.norm()) < 1e-12
    assert float((gl - want_l).norm() / gl.norm()) < 1e-12


def test_dip_term_carries_the_encoder_gradient():
    """With the config's lambdas the DIP term dominates fc_mu's gradient at initialisation: a step
    without it (both lambdas 0) moves that gradient by most of its norm — why the GPU gradient checks
    fail if the DIP seed is missing or wrong."""
    meta, _ = load_case("dipvae_b16")
    sd, x, eps = R.case_inputs(meta)
    full = R.train_step(sd, x, eps, M_N=meta["M_N"], **R.loss_kwargs(meta))
    none = R.train_step(sd, x, eps, M_N=meta["M_N"], lambda_diag=0.0, lambda_offdiag=0.0)
    for name in ("fc_mu.weight",):
        a, b = full["grads"][name].double(), none["grads"][name].double()
        print(name, float((a - b).norm() / a.norm()))
        assert float((a - b).norm() / a.norm()) > 0.5, name
