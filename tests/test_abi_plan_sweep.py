"""tools/abi_plan_sweep.py on the CPU: the table is a function of the library's planning alone (two
runs agree) and of the shapes swept.  (No stored tables: the tool compares two checkouts.)  A
reduced sweep here; the calls with a short workspace are left to the command-line tool."""
import importlib.util
import os

import pytest

from vae_amd import _lib as L

_spec = importlib.util.spec_from_file_location(
    "abi_plan_sweep", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                   "abi_plan_sweep.py"))
sw = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sw)

SMALL = dict(ck=[(32, 64), (256, 512)], ck_ext=[(32, 64)], nk=[(128, 128)], short=False)


@pytest.fixture(scope="module")
def base():
    return sw.table(L, **SMALL)


def test_two_runs_give_the_same_table(base):
    assert sw.table(L, **SMALL) == base
    parts = {r.split()[0] for r in base}
    assert parts == {"base", "ext", "linear", "head"}
    fns = {r.split()[1] for r in base}
    assert fns == set(sw.CONV_FNS + sw.LINEAR_FNS + sw.HEAD_FNS)
    assert any(" rc=0 need=0" in r for r in base) and any(" rc=0 need=" in r and " need=0" not in r for r in base)
    assert any(" rc=-" in r for r in base)                       # rejected calls carry their message


def test_one_changed_k_changes_the_table(base):
    other = sw.table(L, **{**SMALL, "ck": [(32, 64), (256, 256)]})
    assert len(other) == len(base) and other != base
    assert sw.digest(other) != sw.digest(base)
    changed = [a for a, b in zip(base, other) if a != b]
    assert changed and all(r.startswith("base ") and "ck=(256, 512)" in r for r in changed)
