"""The read-only dispatch query conv_fwd_path (host code only: no GPU needed):
which kernel conv_fwd runs a call on, by the launcher's own predicates."""
import itertools

import pytest

from torch_distlearn_amd.ops.conv import (PATH_FIRST_LAYER, PATH_POSM, PATH_REGION_IMAGES, PATH_REGION_ROWS,
                                          PATH_STREAMING, pack_tile)


@pytest.fixture(scope="module")
def C():
    from torch_distlearn_amd import _native

    return _native.native()


IMG = pack_tile(2, region_images=True)
# (B, H, W, Cin, Cout, tile word, splits) -> path
TABLE = [
    ((3, 4, 4, 16, 64, 1, 1), PATH_STREAMING),
    ((3, 4, 4, 8, 64, 2, 1), PATH_STREAMING),                # Cin 8, but H * W is not a multiple of 128
    ((1, 16, 16, 8, 64, 2, 1), PATH_FIRST_LAYER),
    ((1, 16, 16, 8, 64, 2, 2), PATH_STREAMING),              # the first-layer kernel is unsplit
    ((1, 16, 16, 8, 64, 1, 1), PATH_STREAMING),              # ... and tile 2 only
    ((1, 16, 16, 4, 64, pack_tile(2, pair=True), 1), PATH_FIRST_LAYER),
    ((2, 16, 16, 64, 64, 2, 1), PATH_REGION_ROWS),
    ((2, 16, 16, 64, 64, 1, 1), PATH_STREAMING),             # no 64x64 region tile
    ((1, 16, 16, 128, 128, 0, 1), PATH_REGION_ROWS),
    ((1, 16, 16, 256, 64, 2, 1), PATH_STREAMING),            # four channel chunks do not fit
    ((1, 16, 16, 256, 64, 2, 2), PATH_REGION_ROWS),
    ((1, 16, 16, 256, 64, 2, 3), PATH_STREAMING),            # the chunks do not divide by the splits
    ((3, 4, 32, 64, 64, 2, 1), PATH_REGION_ROWS),
    ((3, 8, 8, 64, 64, 2, 1), PATH_STREAMING),
    ((3, 8, 8, 64, 64, IMG, 1), PATH_REGION_IMAGES),
    ((5, 4, 4, 128, 128, IMG, 1), PATH_STREAMING),           # eight images x two chunks exceed the LDS budget
    ((5, 4, 4, 128, 128, IMG, 2), PATH_REGION_IMAGES),
    ((128, 4, 4, 64, 64, 2, 1), PATH_STREAMING | PATH_POSM),
    ((64, 4, 4, 64, 64, 2, 1), PATH_STREAMING),              # the batch is not a multiple of the 128-row tile
    ((64, 4, 4, 64, 64, 1, 1), PATH_STREAMING | PATH_POSM),
    ((128, 4, 8, 64, 64, 2, 2), PATH_STREAMING | PATH_POSM),
    ((128, 16, 16, 64, 64, 1, 1), PATH_STREAMING),           # output not smaller than twice the kernel
    ((128, 4, 4, 32, 64, 2, 1), PATH_STREAMING),             # per-lane taps: never position-major
]


@pytest.mark.parametrize("args,path", TABLE, ids=["-".join(map(str, a)) for a, _ in TABLE])
def test_conv_fwd_path_table(C, args, path):
    B, H, W, cin, cout, tile, splits = args
    assert C.conv_fwd_path(B, H, W, cin, cout, 5, tile, splits) == path
    # stages / waves of the tile word select no other kernel
    assert C.conv_fwd_path(B, H, W, cin, cout, 5, tile | pack_tile(0, stages=2, waves=4), splits) == path


def test_conv_fwd_path_agrees_with_conv_region_ok(C):
    for B, H, W, cin, cout, tile, splits, img in itertools.product(
            (1, 3), (4, 8, 16), (4, 16, 32), (64, 128, 256), (64, 128), (0, 1, 2), (1, 2, 4), (False, True)):
        if cout % (128 if tile == 0 else 64):
            continue
        word = pack_tile(tile, region_images=img)
        region = C.conv_fwd_path(B, H, W, cin, cout, 5, word, splits) in (PATH_REGION_ROWS, PATH_REGION_IMAGES)
        assert region == bool(C.conv_region_ok(B, H, W, cin, cout, 5, word, splits)), (B, H, W, cin, cout, word, splits)


def test_conv_fwd_path_follows_the_process_settings(C):
    try:
        C.set_conv_region(0)
        assert C.conv_fwd_path(2, 16, 16, 64, 64, 5, 2, 1) == PATH_STREAMING
        assert C.conv_fwd_path(1, 16, 16, 8, 64, 5, 2, 1) == PATH_STREAMING
        assert C.conv_fwd_path(3, 8, 8, 64, 64, 5, IMG, 1) == PATH_STREAMING
        C.set_conv_region(2)
        assert C.conv_fwd_path(3, 8, 8, 64, 64, 5, 2, 1) == PATH_REGION_IMAGES
        C.set_conv_region(1)
        C.set_conv_posm(0)
        assert C.conv_fwd_path(128, 4, 4, 64, 64, 5, 2, 1) == PATH_STREAMING
    finally:
        C.set_conv_region(1)
        C.set_conv_posm(1)


def test_conv_fwd_path_rejects_what_conv_fwd_rejects(C):
    with pytest.raises(RuntimeError, match="bad tile id"):
        C.conv_fwd_path(2, 8, 8, 64, 64, 5, 7, 1)
    with pytest.raises(RuntimeError, match="multiple of the N tile"):
        C.conv_fwd_path(2, 8, 8, 64, 64, 5, 0, 1)
    with pytest.raises(RuntimeError, match="pair-packed"):  # a plan the first-layer kernel does not serve
        C.conv_fwd_path(2, 16, 16, 4, 128, 5, pack_tile(0, pair=True), 1)
    with pytest.raises(RuntimeError, match="pair-packed"):  # ... or the 8-channel input
        C.conv_fwd_path(2, 16, 16, 8, 64, 5, pack_tile(2, pair=True), 1)
