"""The row-swapped fp16 image of the 12-wave split training kernel (csrc/hpe_mlp2.hip: img_row,
presplit_tile, img_pos, tr_read8), its two readers, and the packed dz2 table, modelled on the CPU.

Tile row r is stored at image row img_row(r): bits 0-1 and bits 2-3 of r change places, so tile row
16 s + 8 rd + 4 h + q is image row 16 s + 4 q + 2 rd + h.  The four tile rows R0 .. R0 + 3 that one
ds_read_b64_tr_b16 addresses then lie four image rows = 208 dwords = 16 banks apart, and a 32-lane
group's four 16-dword spans tile the 64 banks: 2 LDS cycles per read where adjacent rows took 4
(tests/test_lds_image_tr.py, which models the unswapped image from its own constants).

The transposed read and the bank rules are modelled as in test_lds_image_tr.py / test_lds_layouts.py
(MI355X_MICROARCH.md §LDS: lane groups per instruction, one LDS cycle per group when every bank holds
one distinct address, identical addresses broadcast).  The constants and the address arithmetic below
restate the kernel's.

The last section puts figures on the tile loop's LDS accesses no test modelled before: the head's
partial / label reads, the dz2 and W2 table reads and the A1 park's ds_write2_b32.
"""
import numpy as np
import pytest

from test_lds_layouts import B128_GROUPS, B32_GROUPS, a1_row, cycles

MLP2_FS = 104                  # halves per image row
MLP2_IMG = 3 * 32 * MLP2_FS    # halves per parity: fragments ch, cl, h
MLP2_XS = 100                  # floats per row of the raw tile
SENTINEL = -7.0                # what the image holds where the pre-split never writes
W128_GROUPS = [list(range(8 * g, 8 * g + 8)) for g in range(8)]   # ds_write_b128: 8 x 8 contiguous lanes


def img_row(r):
    """Tile row -> image row (csrc/hpe_mlp2.hip img_row)."""
    return (r & 16) | ((r & 3) << 2) | ((r >> 2) & 3)


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
        d = img_row(r) * MLP2_FS + 48 * h + m0
        img[d:d + 8] = v
        first.append(d)
    return img, first


def tr_addr(kh, lane, s, kb, read):
    """Address (halves, within one fragment) lane supplies to read `read` of K-step s, block kb: the
    lane term img_row(4 h + q) = 4 q + h rows, the K-step 16 s rows, the second read img_row(8) = 2 rows."""
    half, l32 = lane >> 5, lane & 31
    tc = (l32 & 16) + 4 * (l32 & 3)
    row = img_row(4 * half + ((l32 >> 2) & 3)) + 16 * s + img_row(8) * read
    return row * MLP2_FS + img_pos(kh, 32 * kb + tc)


def tr_read(img, addr):
    """ds_read_b64_tr_b16 of one wave: addr[lane] in halves -> out[lane][0..3]."""
    out = np.zeros((64, 4))
    for g in range(4):
        for i in range(16):
            for q in range(4):
                out[16 * g + i][q] = img[addr[16 * g + 4 * q + (i >> 2)] + (i & 3)]
    return out


def test_img_row_is_a_permutation_and_the_readers_terms_are_its_images():
    assert sorted(img_row(r) for r in range(32)) == list(range(32))
    assert all(img_row(img_row(r)) == r for r in range(32))           # bits 0-1 <-> 2-3: an involution
    for s in range(2):
        for rd in range(2):
            for h in range(2):
                for q in range(4):
                    # K-step, second read and lane term add up without carries: immediate offsets
                    assert img_row(16 * s + 8 * rd + 4 * h + q) == 16 * s + 4 * q + 2 * rd + h
                    assert img_row(16 * s + 8 * rd + 4 * h + q) == img_row(16 * s) + img_row(8) * rd + img_row(4 * h + q)


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
    # lane (row r, half h), K-step s, element j <-> channel KH h + 8 s + j (zero from KH on), read at
    # image row img_row(r)
    kh = ((cin + 7) & ~7) // 2
    x = np.random.default_rng(cin + 1).integers(1, 2000, size=(32, cin)).astype(np.float64)
    img, _ = presplit(x, cin)
    for lane in range(64):
        r, h = lane & 31, lane >> 5
        for s in range(6):
            for j in range(8):
                m = 8 * s + j
                want = x[r][kh * h + m] if m < kh and kh * h + m < cin else 0.0
                assert img[img_row(r) * MLP2_FS + 48 * h + m] == want


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
    addr = {lane: (img_row(lane & 31) * MLP2_FS + 48 * (lane >> 5) + 8 * s) // 2 for lane in range(64)}
    assert cycles(addr, B128_GROUPS, 4, 64) == 4


def _tr_cycles(kh, s, kb, rd):
    return cycles({lane: tr_addr(kh, lane, s, kb, rd) // 2 for lane in range(64)}, B32_GROUPS, 2, 64)


def test_transposed_reads_conflict_free_at_48():
    # rows 4 q + h of a 32-lane group start on banks 208 q mod 64 = 0, 16, 32, 48, 16 dwords each
    for s in range(2):
        for kb in range(3):
            for rd in range(2):
                assert _tr_cycles(48, s, kb, rd) == 2


def test_transposed_reads_at_44():
    # KH = 44: the image's gap at position 44 moves the channels from 44 on by 4 positions (2 dwords).
    # Block 0 (channels 0..31) lies before the gap and block 2 (64..95) behind it, pad chunks on the
    # zeros at 92..95: whole, 2 cycles.  Block 1 (32..63) straddles the gap: the group's two 16-column
    # halves are 2 dwords further apart and the rows' spans overlap again, 2-way, 4 cycles
    for s in range(2):
        for rd in range(2):
            assert [_tr_cycles(44, s, kb, rd) for kb in range(3)] == [2, 4, 2]


def test_presplit_stores():
    # ds_write_b128, item i on lane i: eight groups of 8 contiguous lanes, 32 banks.  Tile rows r,
    # r + 1 are image rows 4 apart (16 banks), so a group that crosses a tile row's end lands on
    # the other half of the banks instead of wrapping onto its own first quad: one cycle per group,
    # 8 per wave-instruction (10-11 unswapped), under the 13 cycles of the store's VGPR transfer either way
    _, first = presplit(np.zeros((32, 96)), 96)
    for w in range(6):           # 384 items: six full waves
        addr = {lane: first[64 * w + lane] // 2 for lane in range(64)}
        assert cycles(addr, W128_GROUPS, 4, 32) == 8


# ---- the head tables: dz2 packed [T][3], W2 padded [unit][4] (floats) ----

def test_packed_dz2_reads():
    # the backward: K-step s, k = 2 s + k2, lane half h reads rows 8 k + 4 h .. + 3 as three b128 at
    # (8 k + 4 h) 3 + 0 / 4 / 8; accumulator register g = 4 k + q is row 8 k + 4 h + q, its dZ2[j] element
    # 3 q + j of the twelve.  The head stored dz2[r 3 + j]
    T = 32
    dz2 = np.arange(T * 3)              # value = its own index r 3 + j
    seen = set()
    for h in range(2):
        for k in range(4):
            base = (8 * k + 4 * h) * 3
            assert (base * 4) % 16 == 0 and base + 12 <= T * 3
            t = np.concatenate([dz2[base + 4 * v: base + 4 * v + 4] for v in range(3)])
            for q in range(4):
                g = 4 * k + q
                r = (g & 3) + 8 * (g >> 2) + 4 * h          # the accumulator's row (dz_of)
                for j in range(3):
                    assert t[3 * q + j] == r * 3 + j
                    seen.add(r * 3 + j)
            for v in range(3):                               # broadcast per half: one address per group
                addr = {lane: (8 * k + 4 * (lane >> 5)) * 3 + 4 * v for lane in range(64)}
                assert cycles(addr, B128_GROUPS, 4, 64) == 4
    assert seen == set(range(T * 3))                         # every stored value is read, none twice


def test_w2_table_reads_stay_padded():
    # the head partials: wave w, lane half h dots A1[r][16 h + i] with the W2 row of unit 32 w + 16 h + i,
    # one broadcast b128 per unit of the padded w2t[unit][4]: one address per half-wave, one LDS cycle
    # per lane group.  (Packed [unit][3], twelve reads for sixteen, measured inside the noise: not kept)
    for i in range(16):
        addr = {lane: (16 * (lane >> 5) + i) * 4 for lane in range(64)}
        assert cycles(addr, B128_GROUPS, 4, 64) == 4


def test_own_unit_w2_read_stays_padded():
    # the backward's one own-unit read w2t + tcol 4 (both halves the same 32 rows): conflict-free b128
    addr = {lane: (lane & 31) * 4 for lane in range(64)}
    assert cycles(addr, B128_GROUPS, 4, 64) == 4


# ---- the loop's remaining accesses, per tile and workgroup ----

def test_head_partial_and_label_reads():
    # head_item on thread it < 96 (wave 0 whole, wave 1's first half): r = it / 3, j = it % 3 reads
    # part[(w T + r) 4 + j] for the twelve waves w (paired into ds_read2st64_b32: two b32 accesses) and
    # lab[r 4 + j].  Three of every four dwords are touched, so 32 lanes span 43 dwords and wrap onto
    # their own first banks: 2-way in each 32-lane group.  Wave 0: 4 cycles per b32 access instead of
    # 2, wave 1 (one group): 2 instead of 1 — 13 accesses, 3 extra cycles each: 39 conflict cycles per
    # tile, 5.8 M per launch of the headline step's 147,456 tiles
    for w in range(12):
        a0 = {lane: (w * 32 + lane // 3) * 4 + lane % 3 for lane in range(64)}
        a1 = {lane: (w * 32 + (64 + lane) // 3) * 4 + (64 + lane) % 3 for lane in range(32)}
        assert cycles(a0, B32_GROUPS, 1, 32) == 4
        assert cycles(a1, [list(range(32))], 1, 32) == 2
    # the label of the item, lab[r 4 + j] (the label buffer of the tile's parity, 128 floats each:
    # the same banks in both)
    extra = 12 * ((4 - 2) + (2 - 1))
    for parity in range(2):
        l0 = {lane: parity * 128 + (lane // 3) * 4 + lane % 3 for lane in range(64)}
        l1 = {lane: parity * 128 + ((64 + lane) // 3) * 4 + (64 + lane) % 3 for lane in range(32)}
        assert cycles(l0, B32_GROUPS, 1, 32) == 4
        assert cycles(l1, [list(range(32))], 1, 32) == 2
    extra += (4 - 2) + (2 - 1)
    assert extra == 39
    # the accumulators hacc[tid 4 + 0..2]: one 16-byte aligned b96 per thread, 8 lanes per group at a
    # stride of 4 dwords: conflict-free
    groups96 = [[0, 1, 2, 3, 20, 21, 22, 23], [4, 5, 6, 7, 16, 17, 18, 19],
                [8, 9, 10, 11, 28, 29, 30, 31], [12, 13, 14, 15, 24, 25, 26, 27]]
    groups96 += [[lane + 32 for lane in g] for g in groups96]
    assert cycles({lane: 4 * lane for lane in range(64)}, groups96, 3, 32) == 8


def test_a1_park_write2():
    # the park's sixteen b32 stores pair up as eight ds_write2_b32 (registers g, g + 1: rows a1_row(g),
    # a1_row(g + 1), all 64 lanes contiguous in each): two b32 accesses of 2 LDS cycles, no conflict; the
    # instruction's 6 cycles are its three source dwords' VGPR transfer (MI355X_MICROARCH.md §LDS).  The
    # backward reads the same pairs back as ds_read2_b32
    for g in range(0, 16, 2):
        for gg in (g, g + 1):
            assert cycles({lane: a1_row(gg) + lane for lane in range(64)}, B32_GROUPS, 1, 32) == 2
        assert abs(a1_row(g + 1) - a1_row(g)) <= 255          # one instruction's two dword offsets


def test_modelled_conflict_cycles_per_tile():
    """What the model leaves of SQ_LDS_BANK_CONFLICT per tile and workgroup at KH = 48, against the
    unswapped image: the transposed reads' 36 x 2 x 12 = 864 and the pre-split's 16 are gone; the
    head's 39 stay (5.8 M per launch).  The counter measures 23.5 M per launch: about 120 per tile are
    not named by this model, in which every other access of the loop is conflict-free."""
    swapped = sum(_tr_cycles(48, s, kb, rd) - 2 for s in range(2) for kb in range(3) for rd in range(2))
    assert swapped == 0
    _, first = presplit(np.zeros((32, 96)), 96)
    stores = sum(cycles({lane: first[64 * w + lane] // 2 for lane in range(64)}, W128_GROUPS, 4, 32) - 8
                 for w in range(6))
    assert stores == 0
