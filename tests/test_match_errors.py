"""The argument checks of mavba_match_descriptors (mavmap_amd/csrc/match.hip on batch_call.h), through the C entry point.

The pattern of tests/test_batch_call_errors.py: arguments are judged before the device, so nothing here needs one. The
batch holds two valid items and the bad field is in the SECOND one (the first is judged before it and must not be
written either); the return code and the message of mavba_last_error are part of the contract, and every byte of both
item records and of every pre-filled output array is compared.
"""
import ctypes as C

import numpy as np
import pytest

from mavmap_amd import _abi as A
from tests import test_match_host as TM

NULL = object()
ITEM_MSG = "null or negative argument in match item"

# (field of the second item, its value, what else is set)
CASES = [
    ("n1", -3, {}),
    ("n2", 2 ** 31, {}),
    ("desc2", NULL, {}),
    ("dim", 0, {}),
    ("dim", 6, {}),
    ("dim", 132, {}),
    ("xy1", NULL, {"max_distance": 40.0}),
    ("max_ratio", float("nan"), {}),
]


def _items():
    return [TM.make_item(65, 17, 64, seed=1, max_distance=40.0), TM.make_item(17, 65, 128, seed=2)]


@pytest.mark.parametrize("field,value,also", CASES, ids=["%s-%s" % (c[0], "NULL" if c[1] is NULL else c[1]) for c in CASES])
def test_bad_second_item_is_refused_and_nothing_is_written(mavba, field, value, also):
    arr, outs, hold = TM.c_items(_items())
    for k, v in also.items():
        setattr(arr[1], k, v)
    ctype = dict(type(arr[1])._fields_)[field]
    setattr(arr[1], field, C.cast(None, ctype) if value is NULL else value)
    before = bytes(arr)
    filled = [{k: v.copy() for k, v in o.items()} for o in outs]
    L = mavba.load()
    assert L.mavba_match_descriptors(2, arr, -1) == A.ERR_INVALID_ARGUMENT
    assert L.mavba_last_error().decode() == ITEM_MSG
    assert bytes(arr) == before  # every field of both records, the result fields among them
    for o, f in zip(outs, filled):
        for name in o:
            assert np.array_equal(o[name], f[name]) and np.all(o[name] == TM.FILL), name


def test_the_call_itself(mavba):
    L = mavba.load()
    assert L.mavba_match_descriptors(0, None, -1) == A.OK
    assert L.mavba_match_descriptors(-1, None, -1) == A.ERR_INVALID_ARGUMENT
    assert L.mavba_match_descriptors(1, None, -1) == A.ERR_INVALID_ARGUMENT
    # NULL coordinates are fine without the mask, and an item of no keypoints may leave every pointer NULL
    items = [TM.make_item(17, 16, 64, seed=1, with_xy=False), TM.make_item(0, 0, 64, seed=1, with_xy=False)]
    arr, outs, hold = TM.c_items(items, outputs=())
    arr[1].desc1 = arr[1].desc2 = C.cast(None, C.POINTER(C.c_float))
    before = bytes(arr)
    rc = L.mavba_match_descriptors(2, arr, -1)
    if mavba.device_count() > 0:
        assert rc == A.OK and arr[0].num_matches > 0 and np.isnan(arr[0].median_disparity) and arr[1].num_matches == 0
        return  # (the rest is what a machine without a GPU answers)
    assert rc == A.ERR_NO_DEVICE and "no CPU path" in L.mavba_last_error().decode()  # after the argument checks
    assert bytes(arr) == before
