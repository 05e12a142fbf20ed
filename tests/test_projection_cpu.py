"""--z-projection without a device: the flag, its refusal with feather fusion, the projection store's metadata and the
(channel, row band) deal of a shared region."""
import json
import os

import numpy as np
import pytest

from image_stitcher_amd import omezarr, sharding, stitcher_cli
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters


def test_flag_parses_and_defaults_to_none(tmp_path):
    assert stitcher_cli.parse_args(['-i', str(tmp_path)]).z_projection == 'none'
    for v in ('none', 'max', 'max-only'):
        assert stitcher_cli.parse_args(['-i', str(tmp_path), '--z-projection', v]).z_projection == v
    with pytest.raises(SystemExit):
        stitcher_cli.parse_args(['-i', str(tmp_path), '--z-projection', 'mean'])


def test_flag_reaches_the_stitcher(tmp_path, monkeypatch):
    seen = {}

    class Fake:
        def __init__(self, params, **kw):
            seen.update(kw)

        def run(self):
            seen['ran'] = True

    monkeypatch.setattr(stitcher_cli, 'Stitcher', Fake)
    stitcher_cli.main(['-i', str(tmp_path), '--z-projection', 'max-only'])
    assert seen['z_projection'] == 'max-only' and seen['ran']
    stitcher_cli.main(['-i', str(tmp_path)])
    assert seen['z_projection'] == 'none'


def test_constructor_validates_the_projection(tmp_path):
    params = StitchingParameters(input_folder=str(tmp_path))
    assert Stitcher(params).z_projection == 'none'
    assert Stitcher(params, z_projection='max').z_projection == 'max'
    with pytest.raises(ValueError, match='z_projection'):
        Stitcher(params, z_projection='mean')
    for proj in ('max', 'max-only'):
        with pytest.raises(ValueError, match='overwrite fusion only'):
            Stitcher(params, fusion_mode='feather', z_projection=proj)
    Stitcher(params, fusion_mode='feather')      # without a projection feather stays allowed


def test_cli_refuses_feather_with_a_projection(tmp_path, capsys):
    with pytest.raises(SystemExit) as exc:
        stitcher_cli.main(['-i', str(tmp_path), '--fusion-mode', 'feather', '--z-projection', 'max'])
    assert exc.value.code == 1
    assert 'overwrite fusion only' in capsys.readouterr().err


@pytest.mark.parametrize('levels', [1, 3])
def test_projection_store_metadata(tmp_path, levels):
    path = str(tmp_path / 'R0_stitched_mip.ome.zarr')
    shapes = omezarr.create_store(path, (1, 3, 1, 4343, 3001), np.uint16, pixel_size_um=0.75, dz_um=1.5,
                                  channel_names=['a', 'b', 'c'], channel_colors=[0xFF0000, 0x00FF00, 0x0000FF],
                                  num_levels=levels, chunks=(1, 1, 1, 512, 512), name='R0_t0_mip', compression='blosc')
    want = [(1, 3, 1, 4343 >> lv, 3001 >> lv) for lv in range(levels)]
    assert [tuple(s) for s in shapes] == want
    for lv, shp in enumerate(want):
        with open(os.path.join(path, str(lv), '.zarray')) as fh:
            meta = json.load(fh)
        assert tuple(meta['shape']) == shp and meta['chunks'] == [1, 1, 1, 512, 512]
    with open(os.path.join(path, '.zattrs')) as fh:
        attrs = json.load(fh)
    assert [c['label'] for c in attrs['omero']['channels']] == ['a', 'b', 'c']
    assert len(attrs['multiscales'][0]['datasets']) == levels


@pytest.mark.parametrize('world', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('n_channels,canvas_h,levels', [(1, 4343, 3), (2, 4343, 3), (4, 700, 1), (7, 9000, 2), (3, 100, 1)])
def test_channel_band_deal_covers_every_unit_once(world, n_channels, canvas_h, levels):
    """The projection of a shared region deals (channel, band) units with the stack's helper: whole channels when there
    are at least as many as ranks, else every channel's row bands; together the ranks cover every voxel of every channel
    exactly once."""
    bands = sharding.row_bands(canvas_h, levels)
    cover = np.zeros((n_channels, canvas_h), dtype=np.int64)
    for rank in range(world):
        for c, b in sharding.plane_band_units(n_channels, bands, rank, world):
            y0, y1 = (0, canvas_h) if b < 0 else bands[b]
            cover[c, y0:y1] += 1
    assert (cover == 1).all()
