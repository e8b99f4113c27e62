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


def test_nothing_is_left_stubbed():
    from vae_amd import _lib as L
    call, stream_ptr = L.call, L.stream_ptr
    fp.fingerprint("dropin_eval_b4")
    assert L.call is call and L.stream_ptr is stream_ptr
