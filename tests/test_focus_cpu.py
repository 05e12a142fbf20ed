"""Best-focus projection (--z-projection focus) without a device: the numpy definition against hand-computed cases, and the
validation of the flag, the radius and the refusal with feather fusion."""
import numpy as np
import pytest

from focus_ref import depth_of, focus_reference, focus_score, modified_laplacian
from image_stitcher_amd import native, stitcher_cli
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters


def test_modified_laplacian_clamps_at_the_edges():
    t = np.array([[1, 5, 2]], dtype=np.uint16)
    # x = 0: |2 - 1 - 5| (left neighbour clamps to itself) + |2 - 1 - 1| (one row: both vertical neighbours clamp)
    assert modified_laplacian(t).tolist() == [[4, 7, 3]]
    t = np.array([[1], [5], [2]], dtype=np.uint8)
    assert modified_laplacian(t).tolist() == [[4], [7], [3]]
    t = np.array([[9]], dtype=np.uint16)
    assert modified_laplacian(t).tolist() == [[0]]


@pytest.mark.parametrize('radius,want', [
    (0, [4, 7, 3]),
    (1, [3 * (4 + 4 + 7), 3 * (4 + 7 + 3), 3 * (7 + 3 + 3)]),
    # 2R + 1 = 5 > 3 columns: the window repeats the edge columns, and the one row five times
    (2, [5 * (4 + 4 + 4 + 7 + 3), 5 * (4 + 4 + 7 + 3 + 3), 5 * (4 + 7 + 3 + 3 + 3)]),
])
def test_focus_score_by_hand(radius, want):
    assert focus_score(np.array([[1, 5, 2]], dtype=np.uint16), radius).tolist() == [want]


def test_focus_score_of_a_square():
    rng = np.random.default_rng(3)
    t = rng.integers(0, 65536, (9, 11)).astype(np.uint16)
    ml = modified_laplacian(t)
    for radius in (0, 1, 3, 15):
        want = np.zeros_like(ml)
        for y in range(9):
            for x in range(11):
                ys = np.clip(np.arange(y - radius, y + radius + 1), 0, 8)
                xs = np.clip(np.arange(x - radius, x + radius + 1), 0, 10)
                want[y, x] = ml[np.ix_(ys, xs)].sum()
        np.testing.assert_array_equal(focus_score(t, radius), want)
    assert focus_score(np.array([[0, 65535] * 20] * 40, dtype=np.uint16), 15).max() < 2 ** 32


def test_reference_picks_the_sharpest_plane_and_breaks_ties_by_lowest_z():
    sharp = np.array([[1, 5, 2]], dtype=np.uint16)
    flat = np.full((1, 3), 9, dtype=np.uint16)
    rects = np.array([[0, 0, 1, 3, 0, 1]])        # the tile at canvas columns 1..3 of a 1 x 5 canvas
    # planes z = 3 (sharp), z = 1 (sharp + 10: the same score), z = 0 (flat): the tie between 3 and 1 goes to z = 1
    tiles = np.stack([sharp, sharp + 10, flat])[:, None]
    out, key = focus_reference([(tiles, rects, None, [3, 1, 0])], 1, 5, 0)
    assert out.tolist() == [[0, 11, 15, 12, 0]]
    assert depth_of(key).tolist() == [[-1, 1, 1, 1, -1]]
    assert (key[0, 1:4] >> np.uint64(32)).tolist() == [4, 7, 3] and key[0, 0] == 0
    # the flat plane wins nowhere -- unless it is the only plane: a zero score still makes a key > 0
    out, key = focus_reference([(tiles[2:], rects, None, [4])], 1, 5, 1)
    assert out.tolist() == [[0, 9, 9, 9, 0]] and depth_of(key).tolist() == [[-1, 4, 4, 4, -1]]


def test_reference_windows_use_the_full_tile_not_the_crop():
    """A crop that keeps only column 1 of the tile still scores it with its cropped-away neighbours."""
    t = np.array([[1, 5, 2]], dtype=np.uint16)
    rects = np.array([[0, 1, 1, 1, 0, 0]])
    _, key = focus_reference([(t[None, None], rects, None, [0])], 1, 1, 1)
    assert int(key[0, 0] >> np.uint64(32)) == 3 * (4 + 7 + 3)


def test_reference_over_two_plans_and_gains():
    rng = np.random.default_rng(5)
    th, tw = 6, 7
    a = rng.integers(0, 256, (2, 1, th, tw)).astype(np.uint8)
    b = rng.integers(0, 256, (1, 1, th, tw)).astype(np.uint8)
    gains = rng.uniform(0.5, 2.0, (th, tw)).astype(np.float32)
    ra, rb = np.array([[0, 0, th, tw, 0, 0]]), np.array([[0, 0, th, tw, 2, 3]])
    out, key = focus_reference([(a, ra, [gains, gains], [0, 2]), (b, rb, [gains], [1])], 8, 10, 1)
    from oracle import stitch_oracle as O
    d = depth_of(key)
    assert set(np.unique(d)) <= {-1, 0, 1, 2}
    for z, (tiles, rect, zi) in {0: (a, ra, 0), 2: (a, ra, 1), 1: (b, rb, 0)}.items():
        plane = O.fuse_plane_overwrite([tiles[zi, 0]], rect, 8, 10, gains)
        np.testing.assert_array_equal(out[d == z], plane[d == z])
    assert (out[d == -1] == 0).all() and (d[6:, :3] == -1).all() and (d[:2, 7:] == -1).all() and (d[:6, :7] >= 0).all()


def test_flag_values_and_radius(tmp_path):
    for v in ('none', 'max', 'max-only', 'focus', 'focus-only'):
        assert stitcher_cli.parse_args(['-i', str(tmp_path), '--z-projection', v]).z_projection == v
    assert stitcher_cli.parse_args(['-i', str(tmp_path)]).focus_radius == 3
    assert stitcher_cli.parse_args(['-i', str(tmp_path), '--focus-radius', '15']).focus_radius == 15
    for bad in ('-1', '16', 'x'):
        with pytest.raises(SystemExit):
            stitcher_cli.parse_args(['-i', str(tmp_path), '--focus-radius', bad])


def test_flag_reaches_the_stitcher(tmp_path, monkeypatch):
    seen = {}

    class Fake:
        def __init__(self, params, **kw):
            seen.update(kw)

        def run(self):
            seen['ran'] = True

    monkeypatch.setattr(stitcher_cli, 'Stitcher', Fake)
    stitcher_cli.main(['-i', str(tmp_path), '--z-projection', 'focus-only', '--focus-radius', '5'])
    assert seen['z_projection'] == 'focus-only' and seen['focus_radius'] == 5 and seen['ran']
    stitcher_cli.main(['-i', str(tmp_path)])
    assert seen['z_projection'] == 'none' and seen['focus_radius'] == 3


def test_constructor_validates_focus(tmp_path):
    params = StitchingParameters(input_folder=str(tmp_path))
    s = Stitcher(params, z_projection='focus')
    assert s.z_projection == 'focus' and s.focus_radius == 3
    assert Stitcher(params, z_projection='focus-only', focus_radius=0).focus_radius == 0
    for r in (-1, 16, 2.5):
        with pytest.raises(ValueError, match='focus_radius'):
            Stitcher(params, z_projection='focus', focus_radius=r)
    for proj in ('focus', 'focus-only'):
        with pytest.raises(ValueError, match='overwrite fusion only'):
            Stitcher(params, fusion_mode='feather', z_projection=proj)


def test_cli_refuses_feather_with_focus(tmp_path, capsys):
    with pytest.raises(SystemExit) as exc:
        stitcher_cli.main(['-i', str(tmp_path), '--fusion-mode', 'feather', '--z-projection', 'focus'])
    assert exc.value.code == 1
    assert 'overwrite fusion only' in capsys.readouterr().err


def test_scratch_size_and_entry_points():
    """sq_focus_scratch_bytes: 4 + 1 bytes per tile pixel, each part on 128-byte lines; refusals before any device work."""
    assert native.focus_scratch_bytes(0, 16, 16) == 0
    assert native.focus_scratch_bytes(3, 5, 7) == ((3 * 35 * 4 + 127) // 128 + (3 * 35 + 127) // 128) * 128
    assert native.focus_scratch_bytes(256, 2048, 2048) == 5 * 256 * 2048 * 2048
    with pytest.raises(native.NativeError):
        native.focus_scratch_bytes(-1, 4, 4)
    assert 'sq_fuse_project_focus' in native.EXPORTS and native.lib().sq_version() == 108
