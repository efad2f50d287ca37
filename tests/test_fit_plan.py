"""CPU: hpe_fit_multi_plan, the host-side placement of independent trials in one epoch launch
(csrc/hpe_fit.hip, include/hpe.h): trial i of G_i workgroups gets a lane (blockIdx % 8) and a first
position first_c (blockIdx >> 3) there; block 8 (first_c + c) + lane runs its workgroup c.  The
plan makes no device call, so every property is checked here through ctypes."""
import ctypes

import numpy as np

from hpe import _lib


def _plan(groups, cap):
    lib = _lib.load()
    n = len(groups)
    g = (ctypes.c_int32 * max(n, 1))(*groups)
    lane = (ctypes.c_int32 * max(n, 1))(*([7] * max(n, 1)))
    first = (ctypes.c_int32 * max(n, 1))(*([7] * max(n, 1)))
    k = lib.hpe_fit_multi_plan(g, n, cap, lane, first)
    return k, list(lane)[:n], list(first)[:n]


def _block_map(groups, k, lane, first):
    """The launch's block map rebuilt from the plan: -1 idle, else (trial, c); asserts no overlap."""
    loads = [0] * 8
    for i in range(k):
        loads[lane[i]] = max(loads[lane[i]], first[i] + groups[i])
    grid = 8 * max(loads)
    bmap = [-1] * grid
    for i in range(k):
        for c in range(groups[i]):
            b = 8 * (first[i] + c) + lane[i]
            assert bmap[b] == -1, 'block %d given twice' % b
            bmap[b] = (i, c)
    return bmap, loads


def test_eight_trials_go_one_per_lane():
    k, lane, first = _plan([12] * 8, 32)
    assert k == 8
    assert sorted(lane) == list(range(8))
    assert first == [0] * 8
    bmap, loads = _block_map([12] * 8, k, lane, first)
    assert len(bmap) == 8 * 12 and -1 not in bmap


def test_sixteen_trials_go_two_per_lane():
    k, lane, first = _plan([12] * 16, 32)
    assert k == 16
    assert sorted(lane) == sorted(list(range(8)) * 2)
    for l in range(8):
        assert sorted(first[i] for i in range(16) if lane[i] == l) == [0, 12]
    bmap, loads = _block_map([12] * 16, k, lane, first)
    assert loads == [24] * 8 and len(bmap) == 8 * 24


def test_seventeenth_trial_is_left_over():
    k, lane, first = _plan([12] * 17, 32)
    assert k == 16
    assert lane[16] == -1 and first[16] == -1
    assert all(0 <= l < 8 for l in lane[:16])
    _block_map([12] * 16, k, lane, first)


def test_mixed_widths_stay_within_cap_without_overlap():
    groups = [12, 1, 2, 4, 8, 12, 12]
    k, lane, first = _plan(groups, 32)
    assert k == len(groups)
    bmap, loads = _block_map(groups, k, lane, first)
    assert max(loads) <= 32
    for l in range(8):   # a lane's trials are stacked without gaps: consecutive first_c from 0
        mine = sorted((first[i], groups[i]) for i in range(k) if lane[i] == l)
        pos = 0
        for f, g in mine:
            assert f == pos
            pos += g
    # every workgroup of a trial sits in one lane at consecutive positions
    for i, g in enumerate(groups):
        blocks = [b for b, e in enumerate(bmap) if e != -1 and e[0] == i]
        assert len(blocks) == g
        assert {b % 8 for b in blocks} == {lane[i]}
        assert [b >> 3 for b in blocks] == list(range(first[i], first[i] + g))
    assert sum(e != -1 for e in bmap) == sum(groups)
    # decreasing G, ties in input order: the three G = 12 trials take lanes 0, 1, 2 in input order
    assert [lane[0], lane[5], lane[6]] == [0, 1, 2]


def test_cap_below_some_trial_places_nothing():
    k, lane, first = _plan([2, 12, 4], 8)
    assert k == 0
    assert lane == [-1] * 3 and first == [-1] * 3


def test_no_trials():
    assert _plan([], 32)[0] == 0
    assert _lib.load().hpe_fit_multi_plan(None, 0, 32, None, None) == 0


def test_plan_is_deterministic():
    rng = np.random.default_rng(3)
    groups = [int(g) for g in rng.integers(1, 13, size=40)]
    a = _plan(groups, 32)
    assert a == _plan(groups, 32)
    k, lane, first = a
    assert 1 <= k <= 40
    assert lane[k:] == [-1] * (40 - k) and first[k:] == [-1] * (40 - k)
    bmap, loads = _block_map(groups, k, lane, first)
    assert max(loads) <= 32
    if k < 40:   # a prefix: one more trial in input order would not fit
        assert _plan(groups[:k + 1], 32)[0] == k


def test_table_size_grows_with_trials():
    lib = _lib.load()
    assert lib.hpe_fit_multi_table_size(0) == 0
    s1, s8 = lib.hpe_fit_multi_table_size(1), lib.hpe_fit_multi_table_size(8)
    assert 0 < s1 < s8
    # room for the block map of a launch whose trials all sit in one lane: 8 * 32 blocks per trial
    assert s8 >= 8 * 8 * 32 * 4
