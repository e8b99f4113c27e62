"""Pin the MIWAE restatement (tests/miwae_ref.py) against the reference's golden vectors: the loss
terms at 1e-6 relative, everything else at the bars tests/test_oracle_golden.py uses for the other
models (both sides fp32 ATen on the CPU)."""
import numpy as np
import pytest
import torch

import miwae_ref as R
from golden_util import load_case, rel_err, summary
from oracle import vae_oracle as O


@pytest.mark.parametrize("case", R.CASES)
def test_restatement_matches_reference(case):
    meta, ref = load_case(case)
    sd, x, eps = R.case_inputs(meta)
    M, K = R.case_mk(meta)
    assert meta["samples"] == M * K and meta["estimates"] == M
    out = R.train_step(sd, x, eps, M_N=meta["M_N"], M=M, K=K)
    assert tuple(out["loss"]) == tuple(meta["loss"]) == R.TERMS
    for k, v in meta["loss"].items():
        assert abs(out["loss"][k] - v) <= 1e-6 * abs(v), (k, out["loss"][k], v)
    recon = out["recon"]                                            # [B*M*K, C, H, W], rows b, m, k
    assert recon.shape[0] == meta["batch"] * M * K
    n_head = ref["recon_head"].shape[0]
    assert rel_err(recon[:n_head].numpy(), ref["recon_head"]) < 1e-5
    np.testing.assert_allclose(recon.reshape(recon.shape[0], -1).double().sum(1).numpy(), ref["recon_sum"],
                               rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(out["per_row_mse"].numpy(), ref["per_row_mse"], rtol=1e-5)
    for k in ("mu", "log_var"):
        assert rel_err(out[k].numpy(), ref[k]) < 1e-5, k
    for name in meta["param_names"]:
        if R.pre_bn_bias(name):
            # analytically zero: what either side computes is rounding noise (1e-9 here), and the
            # reference sums the M*K rows of an image through repeat().permute(), the oracle through expand()
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


@pytest.mark.parametrize("B,M,K", [(1, 5, 5), (3, 2, 3), (2, 4, 1), (5, 1, 4)])
def test_closed_form_seeds_are_autograd(B, M, K):
    """The seeds the kernel writes (include/vaehip.h, VAE_LOSS_MIWAE): g_r = w_r (1 + lw_r - Σ_k w lw) /
    (B*M), head_coef = 2 g / img, kl_coef = g * M_N — against fp64 autograd of the loss."""
    g = torch.Generator().manual_seed(100 * B + 10 * M + K)
    img, M_N, D = 48, 0.01, 8
    sse = (img * (0.05 + 2.95 * torch.rand(B * M * K, generator=g))).double()
    mulv = torch.cat([1.3 * torch.randn(B, D, generator=g), 0.5 * torch.randn(B, D, generator=g)], 1).double()
    out, per, hc, kc = R.miwae_elbo64(sse, mulv, M, K, M_N, img)
    lw = (sse / img).view(B, M, K) + M_N * R.kld_rows(mulv).view(B, 1, 1)
    w = torch.softmax(lw, -1)
    wl = (w * lw).sum(-1, keepdim=True)
    gr = (w * (1 + lw - wl) / (B * M)).reshape(-1)
    assert float(out[0]) == pytest.approx(float(wl.mean()), rel=1e-12)
    assert float((hc - gr * 2 / img).norm() / hc.norm()) < 1e-12
    assert float((kc - gr * M_N).norm() / kc.norm()) < 1e-12
    assert torch.equal(per, sse / img)


def test_iwae_at_m_times_k_samples_is_another_objective():
    """One softmax over all M*K rows of an image (IWAE at S = M*K) is not MIWAE: on spread-out
    log-weights the loss and the seeds differ by far more than any bar."""
    g = torch.Generator().manual_seed(3)
    img, B, M, K = 12288, 4, 3, 5
    sse = img * (0.05 + 2.95 * torch.rand(B * M * K, generator=g))
    mulv = torch.cat([1.3 * torch.randn(B, 32, generator=g), 0.5 * torch.randn(B, 32, generator=g)], 1)
    right = R.miwae_elbo64(sse, mulv, M, K, 0.01, img)
    one = R.miwae_elbo64(sse, mulv, M, K, 0.01, img, grouping="all")
    assert abs(float(one[0][0] - right[0][0])) > 5e-3 * abs(float(right[0][0]))
    assert float((one[2] - right[2]).norm() / right[2].norm()) > 0.3
