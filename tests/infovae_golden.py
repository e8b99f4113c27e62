"""The InfoVAE golden cases (tests/golden/infovae_*.npz, written by tests/golden/make_golden_infovae.py):
loading, the inputs rebuilt from the recipe, and the reference restatement's keyword arguments."""
import infovae_ref as R
from golden_util import load_case
from oracle import vae_oracle as O

CASES = ["infovae_imq_b16", "infovae_rbf_b8"]
TERMS = ("loss", "Reconstruction_Loss", "MMD", "KLD")


def case_inputs(meta):
    """(params, x, eps, prior) from the recipe, checked against the fixture's SHA-256s."""
    D = meta["ctor"]["latent_dim"]
    sd = O.make_params(O.vanilla_param_spec(latent_dim=D), meta["seed"])
    x, eps = O.make_inputs(meta["batch"], D, meta["seed"])
    prior = R.make_prior(meta["batch"], D, meta["seed"])
    assert O.sha256_of([x]) == meta["x_sha"], "input recipe drifted"
    assert O.sha256_of([eps]) == meta["eps_sha"], "eps recipe drifted"
    assert O.sha256_of([prior]) == meta["prior_sha"], "prior recipe drifted"
    assert O.sha256_of([sd[k] for k in sd]) == meta["params_sha"], "param recipe drifted"
    return sd, x, eps, prior


def loss_kwargs(meta):
    """Keyword arguments of infovae_ref.train_step / StepPlan(loss='info') for a case (the
    reference constructor's defaults where the case leaves them out)."""
    kw = meta["ctor"]
    return dict(alpha=kw.get("alpha", -0.5), beta=kw.get("beta", 5.0), reg_weight=kw.get("reg_weight", 100),
                kernel_type=kw.get("kernel_type", "imq"), latent_var=kw.get("latent_var", 2.0))


__all__ = ["CASES", "TERMS", "case_inputs", "loss_kwargs", "load_case"]
