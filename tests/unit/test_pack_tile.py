"""ops/conv.py pack_tile: the packed ``tile`` word of the native conv entry
points (layout: csrc/include/dl_ops.h above conv_fwd)."""
import pytest

from torch_distlearn_amd.ops.conv import pack_tile


def test_pack_tile_reproduces_the_call_sites_literals():
    assert pack_tile(2) == 2
    assert pack_tile(2, keep_slabs=True) == 2 | (1 << 20)
    assert pack_tile(2, pair=True) == 2 | (1 << 24)
    for tile in (0, 1, 2):
        assert pack_tile(tile, stages=2, waves=8) == tile | (2 << 4) | (8 << 8)
    assert pack_tile(0, stages=3, waves=4) == 0 | (3 << 4) | (4 << 8)
    assert pack_tile(2, region_images=True) == 2 | (1 << 16)
    assert pack_tile(1, stages=4, waves=8, keep_slabs=True, pair=True, region_images=True) == (
        1 | (4 << 4) | (8 << 8) | (1 << 16) | (1 << 20) | (1 << 24))
    # flags that are false add nothing, whatever their type
    assert pack_tile(2, keep_slabs=0, pair=None, region_images=False) == 2


@pytest.mark.parametrize("stages", [1, 5, 15, -1])
def test_pack_tile_rejects_stages_the_native_decoder_rejects(stages):
    with pytest.raises(ValueError):
        pack_tile(2, stages=stages)


@pytest.mark.parametrize("waves", [1, 2, 6, 16, -4])
def test_pack_tile_rejects_waves_other_than_4_or_8(waves):
    with pytest.raises(ValueError):
        pack_tile(2, waves=waves)


@pytest.mark.parametrize("tile", [-1, 16, 2 | (1 << 20)])
def test_pack_tile_takes_a_plain_tile_id(tile):
    with pytest.raises(ValueError):
        pack_tile(tile)
