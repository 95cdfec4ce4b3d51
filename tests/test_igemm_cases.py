"""The host rules of csrc/conv_igemm.hip as tests/igemm_cases.py restates them, against hand-counted shapes (no GPU): the expectations
tests/test_igemm_gpu.py asserts through mi_debug_last_conv_plan are only as good as these."""
import igemm_cases as C
from igemm_cases import DGRAD, FWD, WGRAD, case


def test_axis_runs():
    # 3 taps, padding 1 on extent 2: position 0 sees taps 1..2, position 1 taps 0..1
    assert C.axis_runs(FWD, 2, 2, 3, 1, 1, 1) == [(0, 1, 1, 2), (1, 1, 0, 2)]
    # extent 1: the centre tap alone
    assert C.axis_runs(FWD, 1, 1, 3, 1, 1, 1) == [(0, 1, 1, 1)]
    # 5 taps, padding 2: extent 3 has three runs, extent 4 a fourth
    assert len(C.axis_runs(FWD, 3, 3, 5, 1, 2, 1)) == 3
    assert C.axis_runs(FWD, 4, 4, 5, 1, 2, 1) is None
    # data gradient, stride 1: input z gets tap a iff 0 <= z + P - a < out
    assert C.axis_runs(DGRAD, 4, 4, 3, 1, 1, 1) == [(0, 1, 0, 2), (1, 2, 0, 3), (3, 1, 1, 2)]


def test_border_rule():
    cls = C.border_classes(FWD, case(3, 2, 2, 2, 32, 32))
    assert cls == [(1, 8)] * 8                                         # 2^3: every voxel a corner, 8 of 27 taps
    assert len(C.border_classes(FWD, case(2, 3, 3, 3, 16, 16, k=5))) == 27
    assert C.border_classes(FWD, case(1, 4, 5, 4, 16, 16, k=5)) is None
    # 0.92: (46 / 48)^2 = 0.918 on 16 x 16, (49 / 51)^2 = 0.923 on 17 x 17
    assert C.border_classes(FWD, case(1, 1, 16, 16, 32, 32, k=(1, 3, 3))) is not None
    assert C.border_classes(FWD, case(1, 1, 17, 17, 32, 32, k=(1, 3, 3))) is None
    assert C.border_classes(DGRAD, case(2, 7, 5, 6, 32, 16, stride=2)) is None
    for c, border in C.BORDER:
        for mode in (FWD, DGRAD):
            assert (C.border_classes(mode, c) is not None) == bool(border), (c, mode)


def test_parity_classes():
    c = case(2, 4, 5, 6, 64, 128, k=1, stride=2)
    assert C.parity_classes(c) == [(2 * 2 * 3 * 3, 1), (2 * 2 * 3 * 3, 0), (2 * 2 * 2 * 3, 0), (2 * 2 * 2 * 3, 0),
                                   (2 * 2 * 3 * 3, 0), (2 * 2 * 3 * 3, 0), (2 * 2 * 2 * 3, 0), (2 * 2 * 2 * 3, 0)]
    assert sum(r for r, _ in C.parity_classes(case(2, 1, 4, 3, 32, 32, stride=2))) == 2 * 1 * 4 * 3
    assert any(r == 0 for r, _ in C.parity_classes(case(2, 1, 4, 3, 32, 32, stride=2)))
    assert sorted(t for _, t in C.parity_classes(case(2, 7, 5, 6, 32, 16, stride=2))) == [1, 2, 2, 2, 4, 4, 4, 8]


def test_plans():
    p = C.expected_plan(FWD, case(16, 8, 8, 8, 16, 16), {"MI_CONV_SPLITS": "4"})
    assert (p["n_classes"], p["row_tiles"], p["col_tiles"], p["bk"], p["fold"]) == (27, 140, 1, 16, 1)
    p = C.expected_plan(DGRAD, case(16, 8, 8, 8, 16, 16, stride=2), {})
    assert (p["n_classes"], p["row_tiles"], p["border"]) == (8, 128, 0)
    for c, mode, splits in C.FOLD:
        p = C.expected_plan(mode, c, {})
        blocks = p["row_tiles"] * p["col_tiles"] * splits
        assert blocks > 512 and blocks % 256, (c, blocks)
    # 64-deep slices only on 128-row tiles; 128-wide tiles only with 32-deep slices; bf16x3 only on 64 x 64
    assert C.expected_plan(FWD, case(1, 1, 5, 7, 128, 128), {"MI_CONV_BK": "64"})["bk"] == 32
    p = C.expected_plan(FWD, case(1, 1, 5, 7, 128, 128), {"MI_CONV_BK": "64", "MI_CONV_BM": "128"})
    assert (p["bm"], p["bn"], p["bk"], p["bf16x3"]) == (128, 64, 64, 0)
    p = C.expected_plan(FWD, case(1, 1, 5, 7, 128, 128), {"MI_CONV_BN": "128", "MI_CONV_BK": "16"})
    assert (p["bn"], p["bk"], p["bf16x3"]) == (64, 16, 1)
    assert C.expected_plan(WGRAD, case(2, 3, 4, 5, 64, 32), {})["wbox"] == 1
    assert C.expected_plan(WGRAD, case(2, 3, 4, 5, 64, 32), {"MI_CONV_BM": "128"})["wbox"] == 0
    assert C.expected_plan(WGRAD, case(2, 3, 4, 5, 48, 32), {})["wbox"] == 0
    for c, switches, wbox in C.WBOX:
        assert C.expected_plan(WGRAD, c, switches)["wbox"] == wbox, (c, switches)
    assert C.expected_plan(FWD, case(2, 5, 6, 7, 1, 16, k=5), {})["stem"] == 1
