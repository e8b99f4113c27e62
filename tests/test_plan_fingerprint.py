"""tools/plan_fingerprint.py on the CPU: the digest of a plan's launches does not depend on where
its buffers land, and does depend on the route the plan takes.  (No stored digests: the tool
compares two checkouts; here it is only checked to be a function of the plan.)"""
import importlib.util
import os

import pytest

_spec = importlib.util.spec_from_file_location(
    "plan_fingerprint", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                     "plan_fingerprint.py"))
fp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fp)


@pytest.fixture(scope="module")
def base():
    return {name: fp.fingerprint(name) for name in ("dropin_train_b4", "vq_b8")}


@pytest.mark.parametrize("name", ["dropin_train_b4", "vq_b8"])
def test_two_builds_give_the_same_digest(base, name):
    import torch
    hold = [torch.empty(n) for n in (1 << 20, 3, 1 << 12)]      # other allocations in between
    assert fp.fingerprint(name) == base[name]
    del hold


@pytest.mark.parametrize("name,flip", [("dropin_train_b4", dict(pad_rgb=False)),
                                       ("dropin_train_b4", dict(batch_wgrads=False)),
                                       ("vq_b8", dict(mat_min_flops=0.0))])
def test_a_route_option_changes_the_digest(base, name, flip):
    assert fp.fingerprint(name, **flip) != base[name]


def test_a_term_changes_the_digest():
    assert fp.fingerprint("info_b16") != fp.fingerprint("info_b16", kernel_type="rbf")
    assert fp.fingerprint("dip_b16") != fp.fingerprint("dip_b16", lambda_diag=1.0)
    assert fp.fingerprint("miwae_b4_m2k3") != fp.fingerprint("miwae_b4_m2k3", estimates=3)


TERM_CONFIGS = ["dip_b16", "miwae_b4_m2k3", "betaB_b16", "info_dropin_b4", "dip_dropin_b4", "miwae_dropin_b2",
                "info_per_op_b16", "dip_fp32_b4", "center_b4"]


@pytest.fixture(scope="module")
def term_plans():
    return {name: fp.build(name)[1] for name in TERM_CONFIGS + ["info_b16"]}


@pytest.mark.parametrize("name", TERM_CONFIGS)
def test_a_plan_has_a_term_exactly_when_it_has_a_fourth_loss_entry(term_plans, name):
    plan = term_plans[name]
    assert (plan.term is None) == (plan.extra_term is None)
    assert (plan.term is not None) == name.startswith(("info", "dip"))
    assert (plan.prior is not None) == name.startswith("info")


def test_an_eval_plan_has_no_term():
    plan = fp.build("info_dropin_b4", training=False)[1]
    assert plan.term is None and plan.extra_term is None and plan.prior is None


@pytest.mark.parametrize("name,queued", [("info_b16", True), ("info_per_op_b16", True), ("dip_b16", True),
                                         ("info_dropin_b4", False), ("dip_dropin_b4", False)])
def test_dropin_term_is_kept_not_queued(term_plans, name, queued):
    """A fused plan runs its term's kernel and the ELBO in the forward; a drop-in plan keeps both for
    loss_function time (the GPU assertion of test_gpu_dipvae_model.py, without a GPU)."""
    plan = term_plans[name]
    fns = [fn for fn, _ in plan.fwd_calls]
    assert (plan.term.fn in fns) == queued and ("vae_elbo_fwd" in fns) == queued
    if not queued:
        assert not any(fn in ("vae_mmd_fwd", "vae_dip_fwd", "vae_elbo_fwd") for fn in fns)


CLOSER_CONFIGS = ["logcosh_b16", "logcosh_per_op_b4", "logcosh_fp32_b4", "logcosh_wide_b4", "mssim_b4",
                  "center_wide_b4", "center_b4"]
NO_CLOSER_CONFIGS = ["logcosh_dropin_b4", "logcosh_eval_b4", "center_eval_b4", "vanilla_b64", "info_b16"]


@pytest.fixture(scope="module")
def closer_plans():
    class Plans(dict):              # (built when first asked for: one broken closer fails its own cases)
        def __missing__(self, name):
            self[name] = fp.build(name)[1]
            return self[name]
    return Plans()


@pytest.mark.parametrize("name", CLOSER_CONFIGS + NO_CLOSER_CONFIGS)
def test_a_fused_training_plan_of_a_closing_loss_ends_its_forward_with_the_closer(closer_plans, name):
    """plan.closer (vae_amd/closers.py) is the forward's last call and the only loss call; it seeds the
    backward through grad_recon, so the head backward carries no ELBO.  Drop-in and eval plans of the
    same losses have no closer, and the log-cosh ones no loss call at all."""
    plan = closer_plans[name]
    fns = [fn for fn, _ in plan.fwd_calls]
    assert (plan.closer is not None) == (name in CLOSER_CONFIGS)
    assert (plan.grad_recon is not None) == plan.seed_recon
    if plan.closer is not None:
        assert plan.fwd_calls[-1][0] == plan.closer.fn and fns.count(plan.closer.fn) == 1
        assert plan.closer.fn == ("vae_logcosh_loss" if name.startswith("logcosh") else "vae_recon_loss")
        assert "vae_elbo_fwd" not in fns and plan.seed_recon and not plan.elbo_in_head
    else:
        assert "vae_logcosh_loss" not in fns and "vae_recon_loss" not in fns
    if name in ("logcosh_dropin_b4", "logcosh_eval_b4"):
        assert "vae_elbo_fwd" not in fns


def _fields(a, skip=()):
    """The non-pointer fields of an argument struct."""
    import ctypes
    return {f: (list(v) if isinstance(v, ctypes.Array) else v) for f, t in a._fields_
            for v in [getattr(a, f)] if t is not ctypes.c_void_p and f not in skip}


@pytest.mark.parametrize("name,skip", [("center_b4", ()), ("mssim_b4", ()), ("logcosh_b16", ("kl_weight", "latent"))])
def test_one_builder_two_callers(closer_plans, name, skip):
    """The closer a plan holds and the one the drop-in builds for tensors of the same shape carry the
    same constants and ask for the same workspace (log-cosh: but for the KL's two, which only a step has)."""
    import torch
    from vae_amd import _lib as L
    plan_kw, held = fp.CONFIGS[name][3], closer_plans[name].closer
    x = torch.zeros(closer_plans[name].B, 3, 64, 64)
    cfg = plan_kw["recon_loss"] if "recon_loss" in plan_kw else plan_kw["alpha"]
    with fp.no_launches(L):
        mine = type(held)(x.shape, x.device, cfg)
    assert type(mine.args) is type(held.args) and _fields(mine.args, skip) == _fields(held.args, skip)
    assert "workspace_bytes" in _fields(mine.args) and mine.args.workspace_bytes == held.args.workspace_bytes > 0
    assert mine.ws.dtype == held.ws.dtype and mine.ws.numel() * mine.ws.element_size() == mine.args.workspace_bytes
    if name == "mssim_b4":      # the defaults of a recon_loss dict, and its own values where it has them
        assert (mine.args.levels, mine.args.normalize, mine.args.window_size) == (5, 1, 11)
        with fp.no_launches(L):
            own = type(held)(x.shape, x.device, {**cfg, "levels": 3, "normalize": False})
        assert (own.args.levels, own.args.normalize) == (3, 0) and own.args.workspace_bytes != mine.args.workspace_bytes


def test_a_closer_argument_changes_the_digest():
    assert fp.fingerprint("logcosh_b16") != fp.fingerprint("logcosh_b16", alpha=20.0)
    mssim = fp.CONFIGS["mssim_b4"][3]["recon_loss"]
    assert fp.fingerprint("mssim_b4") != fp.fingerprint("mssim_b4", recon_loss={**mssim, "normalize": False})


def test_nothing_is_left_stubbed():
    from vae_amd import _lib as L
    call, stream_ptr = L.call, L.stream_ptr
    fp.fingerprint("dropin_eval_b4")
    assert L.call is call and L.stream_ptr is stream_ptr
