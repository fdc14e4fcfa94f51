"""The host side of --detect_tta: the numpy restatement of the eight views (tests/tta_cpu.py) is a group with the header's
table of inverses, its reduction is the float32 sum it claims to be, and the command line refuses the flag without --detect."""
import numpy as np
import pytest

import tta_cpu
from ss25_hierarchical_multiscale_image_classification_amd import main, tta


@pytest.mark.parametrize("side", [7, 224])
def test_the_eight_views_are_distinct_and_inverted_by_the_table(side):
    x = np.random.default_rng(side).integers(0, 256, (2, side, side, 3), dtype=np.uint8)
    views = [tta_cpu.view(x, v) for v in range(8)]  # asserts rot90 form == index form
    assert np.array_equal(views[0], x)
    for a in range(8):
        assert views[a].shape == x.shape and views[a].flags["C_CONTIGUOUS"]
        for b in range(a):
            assert not np.array_equal(views[a], views[b]), (a, b)
        assert np.array_equal(tta_cpu.view(views[a], tta_cpu.INVERSE[a]), x), a
        assert np.array_equal(np.sort(views[a].reshape(2, -1, 3), axis=1), np.sort(x.reshape(2, -1, 3), axis=1))  # a permutation of pixels
    assert tta_cpu.INVERSE == tta.INVERSE == (0, 3, 2, 1, 4, 5, 6, 7)
    assert np.array_equal(views[4], x[:, :, ::-1]) and np.array_equal(views[2], x[:, ::-1, ::-1])
    assert np.array_equal(views[1][0, :, :, 0], np.rot90(x[0, :, :, 0]))


def test_the_restated_reduction():
    pv = np.array([[0.25, 1.0, 0.5, np.nan], [0.75, 1.0, 0.125, 0.5], [0.5, 1.0, 0.25, 0.5]], np.float32)
    mean, rng = tta_cpu.reduce(pv)
    assert mean.dtype == rng.dtype == np.float32
    assert mean[:3].tolist() == [0.5, 1.0, np.float32(np.float32(0.875) / np.float32(3))] and np.isnan(mean[3])
    assert rng[:3].tolist() == [0.5, 0.0, 0.375] and np.isnan(rng[3])
    one_m, one_r = tta_cpu.reduce(pv[1:2])
    assert np.array_equal(one_m, pv[1]) and not one_r.any()
    # the order of the additions is part of the contract: ascending views, not a pairwise or float64 sum
    p = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], np.float32)
    assert tta_cpu.reduce(p)[0][0] == np.float32(1.0) / np.float32(3)
    assert tta_cpu.reduce(p[::-1])[0][0] == np.float32(1.0 + 2.0 ** -23) / np.float32(3)


def test_check_views():
    assert tta.check_views([0, 3, 5]) == (0, 3, 5)
    for bad in ((), (1, 2), (0, 0), (0, 8), (0, -1)):
        with pytest.raises(ValueError):
            tta.check_views(bad)


def test_parser(capsys):
    p = main.build_parser()
    plain = p.parse_args(["--detect"])
    assert plain.detect_tta == "none" and main.tta_views(plain) == (0,)
    assert vars(p.parse_args(["--detect", "--detect_tta", "none"])) == vars(plain)
    main.check_tta_args(p, plain)
    main.check_tta_args(p, p.parse_args([]))
    for mode, views in (("rot4", (0, 1, 2, 3)), ("d4", tuple(range(8)))):
        a = p.parse_args(["--detect", "--detect_tta", mode])
        main.check_tta_args(p, a)
        assert main.tta_views(a) == views == tta.MODES[mode]
        rest = dict(vars(a), detect_tta="none")
        assert rest == vars(plain)  # the flag changes nothing else
    with pytest.raises(SystemExit) as e:
        main.check_tta_args(p, p.parse_args(["--detect_tta", "d4"]))
    assert e.value.code == 2 and "--detect_tta d4 is an option of --detect" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:  # the command itself refuses, before it opens a slide or a device
        main.main(["--detect_tta", "d4", "--patch", "--synthetic", "900,900,1"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        p.parse_args(["--detect", "--detect_tta", "flip"])
    assert e.value.code == 2
