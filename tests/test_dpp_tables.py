"""The lane maps behind the DPP row broadcasts of the 12-wave split training kernel (csrc/hpe_mlp2.hip
BCH, csrc/hpe_dev.h fmac3x4_bcast), modelled on the CPU: the W2 table of the head partials, which the
kernel uses, and the dZ2 table of the backward, which was built, measured slower and is not in the
kernel — its map is kept here so that a later attempt starts from a checked one.

`row_newbcast:N` hands every lane of a 16-lane row the value of lane N of that row
(tests/test_gpu_bcast_probe.py holds the instruction to that on the GPU).  A wave has four rows
q = lane >> 4; rows 0-1 are lane half h = 0, rows 2-3 half h = 1.

  * dZ2 table (backward): lane 16 q + u reads tile row (u & 3) + 8 (u >> 2) + 4 (q >> 1), so broadcast g
    must deliver the row of accumulator register g, (g & 3) + 8 (g >> 2) + 4 h, to all 32 lanes of half h;
  * W2 table (head partials): lane 16 q + u reads unit 16 (q >> 1) + u of the wave's 32, so broadcast u
    must deliver unit 16 h + u to all 32 lanes of half h — the unit whose A1 the lane multiplies there.

The maps are written once more below, as the kernel source has them; the source is checked to still
spell them that way."""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, '..', 'head-pose-estimation-model_amd', 'csrc', 'hpe_mlp2.hip')

LANES = np.arange(64)


def row_newbcast(v, n):
    """v: one value per lane; what each lane sees of v under row_newbcast:n."""
    return v[(LANES & ~15) + n]


def dz2_row_of_lane(lane):
    u, thalf = lane & 15, lane >> 5
    return (u & 3) + 8 * (u >> 2) + 4 * thalf


def w2_unit_of_lane(lane):
    thalf = lane >> 5
    return 16 * thalf + (lane & 15)


def test_dz2_table_delivers_register_rows():
    table = dz2_row_of_lane(LANES)
    for g in range(16):
        seen = row_newbcast(table, g)
        for h in range(2):
            want = (g & 3) + 8 * (g >> 2) + 4 * h      # the row of accumulator register g in half h
            assert (seen[32 * h:32 * h + 32] == want).all(), (g, h)


def test_w2_table_delivers_the_halfs_units():
    table = w2_unit_of_lane(LANES)
    for u in range(16):
        seen = row_newbcast(table, u)
        for h in range(2):
            assert (seen[32 * h:32 * h + 32] == 16 * h + u).all(), (h, u)


def test_every_row_and_unit_is_held():
    assert set(dz2_row_of_lane(LANES)) == set(range(32))
    assert set(w2_unit_of_lane(LANES)) == set(range(32))
    # each twice: the two DPP rows of a lane half hold the same sixteen entries
    assert (np.bincount(dz2_row_of_lane(LANES)) == 2).all()
    assert (np.bincount(w2_unit_of_lane(LANES)) == 2).all()


def test_head_partial_pairs_unit_with_its_activation():
    """The head partial of lane (row r, half h) sums A1[r][16 h + k] * W2[16 h + k] over k = 0 .. 15: the
    k-th activation the lane reads (ar + k: unit 16 h + k of the parked row) meets broadcast k."""
    table = w2_unit_of_lane(LANES)
    for k in range(16):
        a_unit = 16 * (LANES >> 5) + k
        assert (row_newbcast(table, k) == a_unit).all(), k


def test_source_spells_the_maps_this_way():
    s = re.sub(r'\s+', ' ', open(SRC).read())
    assert 'w2t + (wave * 32 + 16 * thalf) * 4' in s and 'wr + (tlane & 15) * 4' in s
