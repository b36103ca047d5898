"""Host side of the shared image prefix: the split scoring.plan_shared_prefix plans, and the new exports of the library."""
import ctypes as C

import pytest
import torch

from llava_reward_amd import _lib, scoring


def _row(n_img, caption, head=(1, 2, 13)):
    return list(head) + [-1] * n_img + [13] + list(caption) + [32000]


def test_plan_on_hand_made_rows():
    rows = [_row(313, [40, 41, 42]), _row(313, [50]), torch.tensor(_row(313, [60, 61]))]          # 3 + 313 + 1 = 317 common tokens
    assert scoring.plan_shared_prefix(rows) == (317, 256)
    rows = [_row(313, [7, 8, 9, 40]), _row(313, [7, 8, 9, 50, 51])]                                # + 3 common caption tokens
    assert scoring.plan_shared_prefix(rows) == (320, 320)
    assert scoring.plan_shared_prefix([_row(313, [7, 8, 9])]) == (321, 320)                         # one row shares all of itself
    n_prefix, n_shared = scoring.plan_shared_prefix([_row(20, [40]), _row(20, [50])])
    assert (n_prefix, n_shared) == (24, 0)                                                          # below one key tile: nothing to cache


def test_plan_refuses_rows_that_do_not_share_their_image():
    with pytest.raises(ValueError, match="image-slot runs differ"):
        scoring.plan_shared_prefix([_row(313, [40]), _row(169, [40])])
    with pytest.raises(ValueError, match="outside the common prefix"):
        scoring.plan_shared_prefix([[1, 5] + [-1] * 70 + [9], [1, 6] + [-1] * 70 + [9]])
    with pytest.raises(ValueError):
        scoring.plan_shared_prefix([])


def test_new_exports_resolve():
    lib = _lib.load()
    for name in ("lr_prefix_bytes", "lr_prefix_build", "lr_forward_prefixed", "lr_op_attention_shared"):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert lib.lr_prefix_bytes(None, 256, 313) == 0                  # no handle: no size, no crash
    assert _lib.PrefixInfo.struct_size.offset == 0 and C.sizeof(_lib.PrefixInfo) == 48
