"""The call-list machinery (vae_amd/calls.py) on fake lists, CPU only: the batching of weight
gradients per backward segment and the struct view of the four entry shapes."""
import ctypes

from vae_amd import _lib as L
from vae_amd.calls import BATCH_FN, batch_filter_calls, structs


def _wg(fn="vae_conv2d_bwd_filter"):
    return (fn, ctypes.byref(L.ConvArgs()))


def _data(fn="vae_conv2d_bwd_data"):
    return (fn, ctypes.byref(L.ConvArgs()))


# (entries compare equal only when they hold the same byref object: == below is identity of the argument)
def _unpad():
    return ("vae_unpad_accumulate", (1, 8, 3, 1 << 24, 1 << 25))


def test_two_segments_get_one_batch_each_at_their_end():
    raw = [_data(), _wg(), _data(), _wg("vae_convT2d_bwd_filter"),       # segment 0: calls [0, 4)
           _wg(), _data(), _wg(), _data()]                               # segment 1: calls [4, 8)
    out, ends = batch_filter_calls(raw, [4, 8])
    assert ends == [3, 6] and len(out) == 6
    assert [fn for fn, _ in out] == ["vae_conv2d_bwd_data", "vae_conv2d_bwd_data", BATCH_FN,
                                     "vae_conv2d_bwd_data", "vae_conv2d_bwd_data", BATCH_FN]
    assert out[0] == raw[0] and out[1] == raw[2] and out[3] == raw[5] and out[4] == raw[7]
    b0, b1 = out[2][1], out[5][1]
    assert b0.calls == [raw[1], raw[3]] and b1.calls == [raw[4], raw[6]]
    assert not b0.side and not b1.side and b0.after == [] and b1.after == []


def test_a_single_weight_gradient_stays_a_call_of_its_own():
    raw = [_data(), _wg(), _data()]
    out, ends = batch_filter_calls(raw, [3])
    assert ends == [3] and [fn for fn, _ in out] == ["vae_conv2d_bwd_data", "vae_conv2d_bwd_data",
                                                     "vae_conv2d_bwd_filter"]
    assert out[2] == raw[1]


def test_unpad_follows_the_batch_that_writes_its_padded_gradient():
    raw = [_wg(), _unpad(), _data(), _wg(), _data()]
    out, ends = batch_filter_calls(raw, [5])
    assert [fn for fn, _ in out] == ["vae_conv2d_bwd_data", "vae_conv2d_bwd_data", BATCH_FN,
                                     "vae_unpad_accumulate"]
    assert ends == [4] and out[3] == raw[1]
    assert out[2][1].calls == [raw[0], raw[3]] and out[2][1].after == []


def test_split_gives_a_side_batch_that_carries_its_unpads():
    raw = [_wg(), _unpad(), _data(), _wg(), _data(), _wg(), _data()]
    out, ends = batch_filter_calls(raw, [7], splits=[4])
    assert [fn for fn, _ in out] == ["vae_conv2d_bwd_data", BATCH_FN, "vae_conv2d_bwd_data", "vae_conv2d_bwd_data",
                                     "vae_conv2d_bwd_filter"]
    side = out[1][1]
    assert side.side and side.calls == [raw[0], raw[3]] and side.after == [raw[1]]
    assert out[4] == raw[5] and ends == [5]            # (one weight gradient left: no batch)


def test_disabled_is_the_identity():
    raw = [_wg(), _unpad(), _data(), _wg()]
    out, ends = batch_filter_calls(raw, [2, 4], splits=[1], enabled=False)
    assert out == raw and out is not raw and ends == [2, 4]


def test_structs_of_every_entry_shape():
    a, rc = L.ConvArgs(n=3), L.ReconArgs(n=5)
    assert structs(None) == []
    assert structs((L.BF16, 1, 3, 8, 1 << 24, None)) == []
    one = structs(ctypes.byref(a))
    assert len(one) == 1 and ctypes.addressof(one[0]) == ctypes.addressof(a)
    two = structs((ctypes.byref(a), ctypes.byref(rc)))
    assert [ctypes.addressof(s) for s in two] == [ctypes.addressof(a), ctypes.addressof(rc)]
    b, c = L.ConvArgs(n=7), L.ConvArgs(n=9)
    batch = L.FilterBatch([("vae_conv2d_bwd_filter", ctypes.byref(b)), ("vae_convT2d_bwd_filter", ctypes.byref(c))])
    assert [s.n for s in structs(batch)] == [7, 9]
    structs(batch)[0].n = 11                                 # the structs themselves, not copies
    assert b.n == 11
