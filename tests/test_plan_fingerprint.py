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


def test_nothing_is_left_stubbed():
    from vae_amd import _lib as L
    call, stream_ptr = L.call, L.stream_ptr
    fp.fingerprint("dropin_eval_b4")
    assert L.call is call and L.stream_ptr is stream_ptr
