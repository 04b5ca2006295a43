"""mavba_triangulate_pairs on the GPU (csrc/triangulate.hip) against the numpy restatement of the reference in
tests/test_triangulate_host.py: positions within the DLT bound measured there, derived quantities at 1e-12, status,
acceptance and compaction for every point, the per-item summaries, bit-reproducibility and NULL outputs.

Sizes: n in {0, 1, 63, 64, 65, 255, 256, 257, 513} - the edges of a wave (64) and of a work-group (256), and an item
of three work-groups whose summaries cross work-groups - alone and mixed in one batch with an empty item in the middle."""
import ctypes as C

import numpy as np
import pytest

from mavmap_amd import _abi as A
from tests import test_triangulate_host as T

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 513)
PAIRS = sorted(T.MODEL_PAIRS)
_cache = {}


def case(n, pair, reject=A.TRI_REJECT_EXTEND):
    """(item, reference, pair record) - generated once, shared by the tests, never modified."""
    key = (n, pair, reject)
    if key not in _cache:
        item = T.make_pair(n, pair, seed=21, reject=reject)
        ref = T.ref_pair(item)
        T.check_generator_preconditions(item, ref)
        _cache[key] = (item, ref, T.pair_record(T.load_host(), item))
    return _cache[key]


def mixed_batch():
    """All sizes and all model pairs in one batch, the empty item in the middle, both reject configurations."""
    order = (513, 1, 64, 255, 0, 257, 63, 256, 65)
    return [case(n, PAIRS[k % 3], A.TRI_REJECT_INITIAL if k % 4 == 3 else A.TRI_REJECT_EXTEND) for k, n in enumerate(order)]


def check_summaries(got, item, ref):
    """mean_folded_angle_deg against numpy's mean of the kernel's OWN angles, at 1e-12 relative: this checks the
    reduction (wave sums, work-group partials, chunk order, the division and the conversion to degrees) and nothing
    else. The angles themselves are tied to the reference per point in check_item, at 1e-12 / sin(angle); the mean of
    the reference's own angles differs from this one by what the positions' DLT bound allows, point by point, and adds
    no check of the sum."""
    n = len(ref["xyz"])
    if n == 0:
        assert got.num_accepted == 0 and np.isnan(got.mean_folded_angle_deg)
        return
    mean = float(np.mean(T.ref_fold(got.angle)) * (180.0 / np.pi))
    assert abs(got.mean_folded_angle_deg - mean) <= 1e-12 * mean, (got.mean_folded_angle_deg, mean)


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("n", SIZES)
def test_single_item_matches_the_reference(mavba, n, pair):
    item, ref, rec = case(n, pair)
    got, = mavba.triangulate_pairs([item])
    T.check_item(got, item, ref, rec, what=f"{pair}/{n}")
    check_summaries(got, item, ref)


@pytest.mark.parametrize("pair", PAIRS)
def test_initial_pair_configuration(mavba, pair):
    """reject_bits = DEPTH1 plus the mean angle: the reference's process_initial (sequential_mapper.cc:302-349)."""
    item, ref, rec = case(257, pair, A.TRI_REJECT_INITIAL)
    got, = mavba.triangulate_pairs([item])
    T.check_item(got, item, ref, rec, what=f"initial {pair}")
    check_summaries(got, item, ref)
    new = ref["has"] == 0
    assert np.array_equal(got.accepted, np.flatnonzero(~new | (ref["depth"][:, 0] > 0)))


def _same_bits(a, b):
    return all(np.array_equal(getattr(a, f).view(np.uint8), getattr(b, f).view(np.uint8))
               for f in ("xyz", "angle", "reproj_error", "depth", "status", "accepted")) \
        and np.array_equal(np.float64(a.mean_folded_angle_deg).view(np.uint64), np.float64(b.mean_folded_angle_deg).view(np.uint64))


def test_mixed_batch_matches_the_reference_and_is_bit_reproducible(mavba):
    cases = mixed_batch()
    items = [c[0] for c in cases]
    first = mavba.triangulate_pairs(items)
    for got, (item, ref, rec) in zip(first, cases):
        T.check_item(got, item, ref, rec, what=f"mixed n={len(ref['xyz'])}")
        check_summaries(got, item, ref)
    # a call gives the same bits twice
    second = mavba.triangulate_pairs(items)
    assert all(_same_bits(a, b) for a, b in zip(first, second))
    # an item gives the same bits alone as inside the batch, and in another place of another batch
    for got, item in zip(first, items):
        alone, = mavba.triangulate_pairs([item])
        assert _same_bits(got, alone), len(item["points2D1"])
    rev = mavba.triangulate_pairs(items[::-1])[::-1]
    assert all(_same_bits(a, b) for a, b in zip(first, rev))


def test_null_outputs_leave_the_others_unchanged(mavba):
    L = mavba.load()
    cases = [case(257, PAIRS[1]), case(0, PAIRS[0]), case(65, PAIRS[2])]
    items = [c[0] for c in cases]
    names = ("xyz", "angle", "reproj_error", "depth", "status", "accepted")
    arr, full, hold = T.c_items(items)
    assert L.mavba_triangulate_pairs(len(items), arr, -1) == A.OK
    summary = [(arr[q].num_accepted, arr[q].mean_folded_angle_deg) for q in range(len(items))]
    for q, (item, ref, rec) in enumerate(cases):
        k = int(arr[q].num_accepted)
        assert np.array_equal(full[q]["accepted"][:k], ref["accepted"]) and np.all(full[q]["accepted"][k:] == -7)
    subsets = [(), ("status",), ("accepted",), ("xyz", "depth"), ("angle", "reproj_error", "accepted"), names[:-1]]
    for keep in subsets:
        arr2, outs, hold2 = T.c_items(items, outputs=keep)
        assert L.mavba_triangulate_pairs(len(items), arr2, -1) == A.OK
        for q in range(len(items)):
            assert arr2[q].num_accepted == summary[q][0]
            assert np.array_equal(np.float64(arr2[q].mean_folded_angle_deg).view(np.uint64), np.float64(summary[q][1]).view(np.uint64))
            for name in names:
                if name in keep:
                    assert np.array_equal(outs[q][name].view(np.uint8), full[q][name].view(np.uint8)), (keep, q, name)
                else:
                    assert np.all(outs[q][name] == -7), (keep, q, name)  # (not passed to the library at all)
    # an item whose outputs are all NULL next to one that wants everything
    arr3, outs3, hold3 = T.c_items(items)
    for name in names:
        setattr(arr3[0], name, C.cast(None, C.POINTER(C.c_int32 if name in ("status", "accepted") else C.c_double)))
    assert L.mavba_triangulate_pairs(len(items), arr3, -1) == A.OK
    assert arr3[0].num_accepted == summary[0][0]
    assert all(np.array_equal(outs3[2][name].view(np.uint8), full[2][name].view(np.uint8)) for name in names)
