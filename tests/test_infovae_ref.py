"""Pin the InfoVAE restatement (tests/infovae_ref.py) against the reference's golden vectors, at the
bars tests/test_oracle_golden.py uses for the other models (both sides fp32 ATen on the CPU)."""
import numpy as np
import pytest

import infovae_ref as R
from golden_util import rel_err, summary
from infovae_golden import CASES, case_inputs, load_case, loss_kwargs
from oracle import vae_oracle as O


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_reference(case):
    meta, ref = load_case(case)
    sd, x, eps, prior = case_inputs(meta)
    out = R.train_step(sd, x, eps, prior, M_N=meta["M_N"], **loss_kwargs(meta))
    assert set(out["loss"]) == set(meta["loss"]) == {"loss", "Reconstruction_Loss", "MMD", "KLD"}
    for k, v in meta["loss"].items():
        assert abs(out["loss"][k] - v) <= 1e-5 * max(abs(v), 1e-3), (k, out["loss"][k], v)
    recon = out["recon"]
    n_head = ref["recon_head"].shape[0]
    assert rel_err(recon[:n_head].numpy(), ref["recon_head"]) < 1e-5
    np.testing.assert_allclose(recon.reshape(recon.shape[0], -1).double().sum(1).numpy(), ref["recon_sum"],
                               rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(out["per_img_mse"].numpy(), ref["per_img_mse"], rtol=1e-5)
    for k in ("mu", "log_var", "z"):
        assert rel_err(out[k].numpy(), ref[k]) < 1e-5, k
    for name in meta["param_names"]:
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


def test_mmd_term_carries_the_encoder_gradient():
    """With the config's parameters the MMD term is nearly all of the encoder's gradient at
    initialisation: a step without it (reg_weight chosen so its coefficient is 0) moves fc_mu's
    gradient by ~1 relative norm — why the GPU gradient checks fail if the term is missing."""
    meta, _ = load_case("infovae_imq_b16")
    sd, x, eps, prior = case_inputs(meta)
    kw = loss_kwargs(meta)
    full = R.train_step(sd, x, eps, prior, M_N=meta["M_N"], **kw)
    none = R.train_step(sd, x, eps, prior, M_N=meta["M_N"], **dict(kw, reg_weight=1.0 - kw["alpha"]))
    for name in ("fc_mu.weight", "fc_var.weight", "encoder.0.0.weight"):
        a, b = full["grads"][name].double(), none["grads"][name].double()
        assert float((a - b).norm() / a.norm()) > 0.9, name
