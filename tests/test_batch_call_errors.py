"""The argument checks the three batched pose calls share (mavmap_amd/csrc/batch_call.h), through the C entry points.

Arguments are judged before the device, so nothing here needs one. The three test_abi_without_a_device tests put one
bad field into a batch of ONE item and look at the return code and at some of its outputs. This file adds what they
leave open: the bad item is the SECOND of two (the first, valid one is judged before it and must not be written
either), the message of mavba_last_error is part of the contract, every byte of both item records is compared, not a
choice of result fields, and the table holds (field, value) pairs those tests do not have: per call a negative n, a NULL
required pointer with n > 0, camera model 0 and 4, and for the RANSAC calls a repeated index and an index equal to n in
the first and in the last supplied row.
"""
import ctypes as C

import numpy as np
import pytest

from mavmap_amd import _abi as A
from tests import test_absolute_pose_host as TA
from tests import test_relative_pose_host as TR
from tests import test_triangulate_host as TT

NULL = object()
ITEM_MSG = "null or negative argument in %s item"
MODEL_MSG = "bad camera model"
ROW_MSG = "sample row with a repeated or out-of-range index"
N = 65  # points per item, so 65 is the first index out of range
TRIALS = 20


def _tri_items():
    return [TT.make_pair(N, "opencv_cata", seed=1), TT.make_pair(N, "pinhole_pinhole", seed=2)]


def _abs_items():
    return [TA.make_item(N, A.MODEL_OPENCV, seed=1, max_trials=TRIALS, supplied=True),
            TA.make_item(N, A.MODEL_PINHOLE, seed=2, max_trials=TRIALS, supplied=True)]


def _rel_items():
    return [TR.make_item(N, A.MODEL_OPENCV, A.MODEL_PINHOLE, seed=1, max_trials=TRIALS, supplied=True),
            TR.make_item(N, A.MODEL_PINHOLE, A.MODEL_CATA, seed=2, max_trials=TRIALS, supplied=True)]


# call: (entry point, the two valid items, c_items with every output and result field pre-filled, what the message calls an item)
CALLS = {
    "triangulate": ("mavba_triangulate_pairs", _tri_items, lambda items: TT.c_items(items), "triangulation"),
    "absolute": ("mavba_absolute_pose_ransac", _abs_items, lambda items: TA.c_items(items, fill=-7), "absolute-pose"),
    "relative": ("mavba_relative_pose_ransac", _rel_items, lambda items: TR.c_items(items, fill=-7), "relative-pose"),
}

# (call, field of the second item, its value, return code, message); a field "samples[t]" replaces row t of the supplied rows
CASES = [
    ("triangulate", "n", -3, A.ERR_INVALID_ARGUMENT, ITEM_MSG),
    ("triangulate", "n", 2 ** 31, A.ERR_INVALID_ARGUMENT, ITEM_MSG),
    ("triangulate", "intrinsics1", NULL, A.ERR_INVALID_ARGUMENT, ITEM_MSG),
    ("triangulate", "camera_model1", 4, A.ERR_BAD_MODEL, MODEL_MSG),
    ("triangulate", "camera_model2", 0, A.ERR_BAD_MODEL, MODEL_MSG),
    ("absolute", "n", -3, A.ERR_INVALID_ARGUMENT, ITEM_MSG),
    ("absolute", "xyz", NULL, A.ERR_INVALID_ARGUMENT, ITEM_MSG),
    ("absolute", "camera_model", 0, A.ERR_BAD_MODEL, MODEL_MSG),
    ("absolute", "camera_model", 4, A.ERR_BAD_MODEL, MODEL_MSG),
    ("absolute", "samples[0]", [5, 2, 9, 5], A.ERR_INVALID_ARGUMENT, ROW_MSG),
    ("absolute", "samples[%d]" % (TRIALS - 1), [7, 7, 1, 2], A.ERR_INVALID_ARGUMENT, ROW_MSG),
    ("absolute", "samples[0]", [N, 0, 1, 2], A.ERR_INVALID_ARGUMENT, ROW_MSG),
    ("relative", "n", -3, A.ERR_INVALID_ARGUMENT, ITEM_MSG),
    ("relative", "uv2", NULL, A.ERR_INVALID_ARGUMENT, ITEM_MSG),
    ("relative", "camera_model1", 4, A.ERR_BAD_MODEL, MODEL_MSG),
    ("relative", "camera_model2", 0, A.ERR_BAD_MODEL, MODEL_MSG),
    ("relative", "samples[0]", [1, 2, 3, 4, 1], A.ERR_INVALID_ARGUMENT, ROW_MSG),
    ("relative", "samples[%d]" % (TRIALS - 1), [0, 1, 2, 3, 3], A.ERR_INVALID_ARGUMENT, ROW_MSG),
    ("relative", "samples[0]", [0, N, 1, 2, 3], A.ERR_INVALID_ARGUMENT, ROW_MSG),
]


@pytest.mark.parametrize("call,field,value,code,message", CASES, ids=["%s-%s-%s" % (c[0], c[1], "NULL" if c[2] is NULL else c[2]) for c in CASES])
def test_bad_second_item_is_refused_and_nothing_is_written(mavba, call, field, value, code, message):
    entry, make, c_items, what = CALLS[call]
    items = make()
    if field.startswith("samples["):
        rows = items[1]["samples"].copy()
        rows[int(field[8:-1])] = value
        items[1] = dict(items[1], samples=rows)
    arr, outs, hold = c_items(items)
    if not field.startswith("samples["):
        ctype = dict(type(arr[1])._fields_)[field]
        setattr(arr[1], field, C.cast(None, ctype) if value is NULL else value)
    before = bytes(arr)
    filled = [{k: v.copy() for k, v in o.items()} for o in outs]
    L = mavba.load()
    assert getattr(L, entry)(2, arr, -1) == code
    assert L.mavba_last_error().decode() == (message % what if "%s" in message else message)
    assert bytes(arr) == before  # every field of both records, the result fields among them
    for o, f in zip(outs, filled):
        for name in o:
            assert np.array_equal(o[name], f[name]) and np.all(o[name] == (-7 % 256 if o[name].dtype == np.uint8 else -7)), name
