"""Independent reference of the crop / flip augmentation (numpy, CPU only).

``augment_image`` never computes a source index per pixel as the kernel and
``DeviceLoader.getBatch`` do: it zero-pads the image, cuts the window at
``(dy, dx)`` and mirrors the window.  With P(i, j) = src(i - pad, j - pad) the
window is C(h, w') = P(h + dy, w' + dx) = src(h + dy - pad, w' + dx - pad) and
the output is out(h, w) = C(h, W-1-w if flip else w): the contract's
src(h + dy - pad, (W-1-w if flip else w) + dx - pad), zero outside the image.
"""
import numpy as np


def augment_image(x, flip: int, dx: int, dy: int, pad: int):
    """x [H, W, ...] -> the augmented image, same shape and dtype; the fill is
    the dtype's zero (bit pattern 0 for the uint16 views of bf16 buffers)."""
    x = np.asarray(x)
    H, W = x.shape[:2]
    big = np.zeros((H + 2 * pad, W + 2 * pad) + x.shape[2:], x.dtype)
    big[pad:pad + H, pad:pad + W] = x
    win = big[dy:dy + H, dx:dx + W]
    return win[:, ::-1].copy() if flip else win.copy()


def augment_batch(x, params, pad: int):
    """x [B, H, W, ...], params = B (flip, dx, dy) triples."""
    assert len(params) == len(x)
    return np.stack([augment_image(x[b], *params[b], pad) for b in range(len(x))])


def triples(pad: int, flip: bool = True):
    """Every (flip, dx, dy) a draw can produce."""
    n = 2 * pad + 1
    return {(f, dx, dy) for f in ((0, 1) if flip else (0,)) for dx in range(n) for dy in range(n)}
