"""The one fp16 image per X tile of the 12-wave split training kernel (csrc/hpe_mlp2.hip: presplit_tile,
img_pos, tr_read8) and its two readers, modelled on the CPU:

  * the forward's row reads (ds_read_b128, one per K-step and fragment), and
  * dW1's A operand X^T read from the SAME image with ds_read_b64_tr_b16.

The transposed read is modelled as cdna_hip_programming.md T10 states it: per group of 16 consecutive
lanes, lane 4 q + p supplies the address of row q, columns 4 p .. 4 p + 3 of a 4-row x 16-column block of
16-bit values, and lane i receives column i of the four rows, row q in its element q.  The bank rules
are MI355X_MICROARCH.md §LDS's (test_lds_layouts.cycles): ds_read_b64_tr_b16 is served in two 32-lane
groups over 64 banks, ds_write_b128 in eight groups of 8 contiguous lanes over 32 banks.

The constants and the address arithmetic below restate the kernel's.
"""
import numpy as np
import pytest

from test_lds_layouts import B128_GROUPS, B32_GROUPS, cycles

MLP2_FS = 104                  # halves per image row
MLP2_IMG = 3 * 32 * MLP2_FS    # halves per parity: fragments ch, cl, h
MLP2_XS = 100                  # floats per row of the raw tile
SENTINEL = -7.0                # what the image holds where the pre-split never writes


def img_pos(kh, c):
    """Position (halves) of channel c in an image row (csrc/hpe_mlp2.hip img_pos)."""
    if kh == 48:
        return c
    return c if c < kh else min(c + 48 - kh, 92)


def presplit(x, cin):
    """One fragment of the image as presplit_tile writes it: 384 items of 8 halves, from the raw tile
    (row stride MLP2_XS, pad channels [cin, 96) zero).  Returns the image and, per item, the first
    half written (for the store's bank model)."""
    kh = ((cin + 7) & ~7) // 2
    raw = np.full((32, MLP2_XS), 99.0)      # floats past 96 of a raw row are never read
    raw[:, :96] = 0.0
    raw[:, :cin] = x
    img = np.full(32 * MLP2_FS, SENTINEL)
    first = []
    for i in range(32 * 12):
        r, rem = divmod(i, 12)
        h = 1 if rem >= 6 else 0
        m0 = 8 * (rem - 6 * h)
        s = kh * h + m0
        v = list(raw[r, s:s + 4]) + (list(raw[r, s + 4:s + 8]) if m0 + 4 < kh else [0.0] * 4)
        d = r * MLP2_FS + 48 * h + m0
        img[d:d + 8] = v
        first.append(d)
    return img, first


def tr_addr(kh, lane, s, kb, read):
    """Address (halves, within one fragment) lane supplies to read `read` of K-step s, block kb."""
    half, l32 = lane >> 5, lane & 31
    tc = (l32 & 16) + 4 * (l32 & 3)
    row = 16 * s + 8 * read + 4 * half + ((l32 >> 2) & 3)
    return row * MLP2_FS + img_pos(kh, 32 * kb + tc)


def tr_read(img, addr):
    """ds_read_b64_tr_b16 of one wave: addr[lane] in halves -> out[lane][0..3]."""
    out = np.zeros((64, 4))
    for g in range(4):
        for i in range(16):
            for q in range(4):
                out[16 * g + i][q] = img[addr[16 * g + 4 * q + (i >> 2)] + (i & 3)]
    return out


@pytest.mark.parametrize('cin', [96, 88])
def test_transposed_reads_deliver_the_dw1_operand(cin):
    kh = ((cin + 7) & ~7) // 2
    x = np.random.default_rng(cin).integers(1, 2000, size=(32, cin)).astype(np.float64)
    img, _ = presplit(x, cin)
    for s in range(2):
        for kb in range(3):
            got = np.concatenate([tr_read(img, [tr_addr(kh, lane, s, kb, rd) for lane in range(64)])
                                  for rd in range(2)], axis=1)
            for lane in range(64):
                h, m = lane >> 5, lane & 31
                for j in range(8):
                    row, c = 16 * s + 8 * (j >> 2) + 4 * h + (j & 3), 32 * kb + m
                    want = x[row][c] if c < cin else 0.0
                    assert got[lane][j] == want, (cin, s, kb, lane, j)


@pytest.mark.parametrize('cin', [96, 88])
def test_forward_rows_of_the_same_image(cin):
    # lane (row r, half h), K-step s, element j <-> channel KH h + 8 s + j (zero from KH on)
    kh = ((cin + 7) & ~7) // 2
    x = np.random.default_rng(cin + 1).integers(1, 2000, size=(32, cin)).astype(np.float64)
    img, _ = presplit(x, cin)
    for lane in range(64):
        r, h = lane & 31, lane >> 5
        for s in range(6):
            for j in range(8):
                m = 8 * s + j
                want = x[r][kh * h + m] if m < kh and kh * h + m < cin else 0.0
                assert img[r * MLP2_FS + 48 * h + m] == want


@pytest.mark.parametrize('kh', [48, 44])
def test_transposed_addresses_aligned_and_in_bounds(kh):
    for s in range(2):
        for kb in range(3):
            for rd in range(2):
                for f in range(3):
                    for lane in range(64):
                        a = f * 32 * MLP2_FS + tr_addr(kh, lane, s, kb, rd)
                        assert a % 4 == 0                      # 8 bytes
                        assert 0 <= a and a + 4 <= MLP2_IMG    # inside the parity buffer
                        # the four halves lie in one row's 96 written positions
                        assert (a % MLP2_FS) + 4 <= 96
    assert (MLP2_IMG * 2) % 16 == 0 and (32 * MLP2_FS * 2) % 16 == 0   # parity / fragment bases


@pytest.mark.parametrize('s', range(6))
def test_forward_reads_stay_conflict_free(s):
    addr = {lane: ((lane & 31) * MLP2_FS + 48 * (lane >> 5) + 8 * s) // 2 for lane in range(64)}
    assert cycles(addr, B128_GROUPS, 4, 64) == 4


@pytest.mark.parametrize('kh', [48, 44])
def test_transposed_reads_two_way(kh):
    # stride 104 halves = 52 dwords: rows R0 + q, q = 0..3, of a 32-lane group start on banks
    # 52 q mod 64 = 0, 52, 40, 28 and each spans 16 dwords (the group's two 16-column blocks), so
    # neighbouring rows overlap in 4 banks: 2-way, 4 LDS cycles per wave-instruction instead of 2
    for s in range(2):
        for kb in range(3):
            for rd in range(2):
                addr = {lane: tr_addr(kh, lane, s, kb, rd) // 2 for lane in range(64)}
                assert cycles(addr, B32_GROUPS, 2, 64) == 4


def test_presplit_stores():
    # ds_write_b128, item i on lane i: eight groups of 8 contiguous lanes, 32 banks.  Eight items of
    # one row cover 32 contiguous dwords (one cycle); a group that crosses a row end (every third
    # one: 12 items per row) skips the 4 pad dwords there and wraps onto its own first bank quad:
    # 2-way, 2 cycles.  10 or 11 LDS-array cycles per wave-instruction, under the 13 cycles the
    # store's VGPR transfer takes anyway (MI355X_MICROARCH.md §LDS), so the conflicts cost no time
    _, first = presplit(np.zeros((32, 96)), 96)
    groups = [list(range(8 * g, 8 * g + 8)) for g in range(8)]
    total = 0
    for w in range(6):           # 384 items: six full waves
        addr = {lane: first[64 * w + lane] // 2 for lane in range(64)}
        c = cycles(addr, groups, 4, 32)
        assert c in (10, 11)
        total += c
    assert total == 48 + 16
