"""View augmentation, host side: the tests' numpy restatement of the chain (tests/augment_ref.py) against what PIL makes
of the same records (tests/golden/augment2d.npz, written by tests/golden/gen_golden_augment.py), the Philox restatement
against the generator's published known answers, and the flag's default."""
import numpy as np
import pytest

import augment_ref as R

FIELDS = ("hflip", "vflip", "bright_first", "brightness", "contrast", "s", "i", "j", "k")


def fixture_records(z, b):
    return {k: z["%s_%d" % (k, b)] for k in FIELDS + ("cls",)}


@pytest.mark.parametrize("bbox", [36, 32])
def test_restatement_reproduces_the_pil_fixture(golden, bbox):
    """Flips and rotation only (class 0): exact.  Jitter without a resize (class 1): exact too - the blends are the
    library's own single-precision operations.  With a resize: within 1 grey level, every pixel - the library interpolates
    in two passes with an 8-bit intermediate (each pass at most half a level off), the restatement in one."""
    z = golden("augment2d.npz")
    r = fixture_records(z, bbox)
    assert sorted(np.bincount(r["cls"]).tolist()) == [8, 8, 8, 8]
    combos = {(int(r["hflip"][n]), int(r["vflip"][n]), int(r["bright_first"][n]), int(r["k"][n])) for n in range(32)}
    assert len(combos) == 32                                            # every flag combination with every k
    worst = 0
    for n in range(32):
        got = R.chain_levels(z["crops_%d" % bbox][n], *[r[k][n] for k in FIELDS])
        d = np.abs(got.astype(np.int32) - z["views_%d" % bbox][n].astype(np.int32))
        assert (r["s"][n] == bbox) == (r["cls"][n] < 2) and ((r["brightness"][n] == 1) and (r["contrast"][n] == 1)) == (r["cls"][n] % 2 == 0)
        assert d.max() <= (0 if r["cls"][n] < 2 else 1), (bbox, n, int(r["cls"][n]), int(d.max()))
        worst = max(worst, int(d.max()))
    print("bbox %d: worst difference %d level" % (bbox, worst))


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32_10."""
    hexes = lambda v: [int(x) for x in v]
    assert hexes(R.philox4x32_10(0, 0, 0, 0, 0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert hexes(R.philox4x32_10(f, f, f, f, f, f)) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert hexes(R.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_table_layout_round_trip():
    rec = R.draw_records(np.arange(100), 317, 0, 0, 36)
    back = R.unpack_params(R.pack_params(**rec))
    for k, v in rec.items():
        assert np.array_equal(back[k], v), k


def test_augment_flag_defaults_to_mirror():
    from cet_pick_amd.opts import opts
    assert opts().parse(["simsiam3d"]).augment == "mirror"
    assert opts().parse(["simsiam3d", "--augment", "reference"]).augment == "reference"
    with pytest.raises(SystemExit):
        opts().parse(["simsiam3d", "--augment", "none"])


def test_wrapper_has_no_cpu_path():
    import torch
    from cet_pick_amd import _lib
    from cet_pick_amd.datasets import augment as A
    with pytest.raises(_lib.HipExtensionError):
        A.draw_params(torch.arange(4), 317, 0, 0, 36)
    with pytest.raises(_lib.HipExtensionError):
        A.apply(torch.zeros(4, 36, 36), torch.arange(4), torch.zeros(4, 8, dtype=torch.int32), 0.0, 1.0)
