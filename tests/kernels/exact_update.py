"""Bit-exact references for the fused SGD update, the split-K slab sums it
consumes, the first-layer pack and the next-step gather (csrc/kernels
sgd_dev.h, slab_reduce_dev.h, prep_dev.h, flat_ops.hip).

numpy on the CPU only.  Every function models the arithmetic of the device
code from its documented contract -- which operations are rounded, and in
which order sums associate -- never its index arithmetic or its loops:

* ``fma32``: the correctly rounded fp32 fused multiply-add.
* ``sgd_ref``: one element update, three explicit fmas (sgd_elem).
* ``slab_sum_ref``: strided lanes in split order, then an xor butterfly.
* ``pack1_index_ref``: the packed first-layer layouts of dl_common.h.
* ``gather_ref`` / ``gather_allowed``: the gathered, normalised batch in fp64
  and the bf16 values a correct fp32 evaluation of it may produce.

Exact regime: small integers and dyadic constants make every intermediate an
fp32 number, so the result is the formula in fp64 in any order
(``sgd_formula64``) and a difference is an indexing, range or scale mistake.
Real regime: the same references are bitwise for real-valued data.
"""
from __future__ import annotations

import numpy as np

F32, F64, U32 = np.float32, np.float64, np.uint32


# --------------------------------------------------------------------------- fp32 fma
def fma32(a, b, c):
    """fp32(a * b + c) with ONE rounding, elementwise over fp32 arrays.

    The product of two fp32 numbers has at most 48 significant bits: exact in
    fp64.  s = fl64(p + c) with Knuth's TwoSum gives the exact error term; if
    the sum is inexact, the fp64 result is replaced by the one of the two
    neighbouring doubles around the true value whose last mantissa bit is odd
    (round-to-odd).  53 >= 2 * 24 + 2 bits, so rounding that to fp32 equals
    rounding the true value once.  ``fp32(fp64(a * b + c))`` is not this: it
    rounds twice (tests/unit/test_exact_oracle.py has the case)."""
    a, b, c = (np.asarray(v, dtype=F32).astype(F64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    step = (err != 0) & even & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(step, np.nextafter(s, toward), s)
    return s.astype(F32)


def f32(x):
    return np.asarray(x, dtype=F64).astype(F32)


def mul32(a, b):
    """fp32(a * b): the fp64 product of fp32 operands is exact, one rounding."""
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64)).astype(F32)


def add32(a, b):
    """fp32(a + b): the fp64 sum of two fp32 numbers rounds to fp32 as the
    exact sum does (53 >= 2 * 24 + 2)."""
    return (np.asarray(a, F32).astype(F64) + np.asarray(b, F32).astype(F64)).astype(F32)


# --------------------------------------------------------------------------- bf16
def bf16_bits(x):
    """Round-to-nearest-even bf16 bit patterns (uint16) of fp32 values, in
    integer arithmetic: add 0x7fff plus the lowest kept bit, drop 16 bits.
    NaN -> the quiet NaN 0x7fc0 (the integer rule alone could carry a
    signalling NaN's payload into the exponent)."""
    u = np.ascontiguousarray(np.asarray(x, dtype=F32)).view(U32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(np.asarray(x, dtype=F32)), np.uint16(0x7FC0), r)


def bf16_widen(bits):
    """bf16 bit patterns -> fp32 (a 16-bit shift)."""
    return (np.asarray(bits, dtype=np.uint16).astype(U32) << 16).view(F32)


def bf16_round64(x):
    """fp64 values rounded ONCE to the nearest bf16 (ties to even), returned
    as fp64.  Normal range only (asserted)."""
    x = np.asarray(x, dtype=F64)
    m, e = np.frexp(x)  # x = m 2^e, 0.5 <= |m| < 1
    assert np.all((x == 0) | ((e > -120) & (e < 120)))
    return np.ldexp(np.rint(m * 256.0), e - 8)  # rint: ties to even; 8 significant bits


# --------------------------------------------------------------------------- the element update
def participation_scale(count):
    """s of sgd_elem: fp32(1) / fp32(n) correctly rounded when n > 1, else 1."""
    n = F32(count)
    return F32(F64(1.0) / F64(n)) if n > F32(1.0) else F32(1.0)


def sgd_ref(p, g, m, s, wd, lr, mu):
    """(p', m') of sgd_elem: gx = fma(g, s, fp32(wd p)); with momentum
    (m is not None) mv = fma(mu, m, gx) is the new momentum and the step;
    p' = fma(-lr, step, p).  All arguments fp32."""
    p, g = np.asarray(p, F32), np.asarray(g, F32)
    gx = fma32(g, F32(s), mul32(F32(wd), p))
    m2 = None
    if m is not None:
        gx = m2 = fma32(F32(mu), np.asarray(m, F32), gx)
    return fma32(-F32(lr), gx, p), m2


def sgd_formula64(p, g, m, count, wd, lr, mu):
    """The update as a formula in fp64 (exact regime: equals sgd_ref)."""
    p, g = np.asarray(p, F64), np.asarray(g, F64)
    d = g / (count if count > 1 else 1.0) + wd * p
    m2 = None
    if m is not None:
        d = m2 = mu * np.asarray(m, F64) + d
    return p - lr * d, m2


# --------------------------------------------------------------------------- slab sums
def slab_tpo(splits: int) -> int:
    """Lanes per output of a slab sum: 1 below 8 splits, 8 for 8..31, 32 from 32."""
    return 32 if splits >= 32 else 8 if splits >= 8 else 1


def slab_sum_ref(slabs, tpo: int):
    """Sum over axis 0 of fp32 ``slabs[splits, len]`` in the kernels' order:
    lane t of ``tpo`` starts from 0.f and adds splits t, t + tpo, ... in
    order; then for o = tpo/2 .. 1 every lane t adds lane t ^ o; lane 0's
    value.  For tpo 8: ((p0+p4)+(p2+p6)) + ((p1+p5)+(p3+p7))."""
    slabs = np.asarray(slabs, dtype=F32)
    assert slabs.ndim == 2 and tpo in (1, 8, 32)
    part = []
    for t in range(tpo):
        acc = np.zeros(slabs.shape[1], dtype=F32)
        for sp in range(t, slabs.shape[0], tpo):
            acc = add32(acc, slabs[sp])
        part.append(acc)
    o = tpo // 2
    while o > 0:
        part = [add32(part[t], part[t ^ o]) for t in range(tpo)]
        o //= 2
    return part[0]


# --------------------------------------------------------------------------- first-layer pack
def pack1_size(cout: int, taps: int, cp: int) -> int:
    """Elements of the packed buffer: [Cout][taps][cp], or for cp = -KW
    [Cout][KW][ceil(KW/2)][2][4]."""
    if cp > 0:
        return cout * taps * cp
    kw = -cp
    assert taps == kw * kw
    return cout * kw * ((kw + 1) // 2) * 2 * 4


def pack1_index_ref(e, C: int, cp: int):
    """Where element e of a [Cout][taps][C] weight lies in the packed buffer.
    cp > 0: channel c of pixel px = (co, tap) sits at [px][c] of [.][cp].
    cp = -KW: tap (kh, kx) of output channel co sits in chunk kx // 2 of row
    kh, half kx % 2, channel c of [Cout][KW][ceil(KW/2)][2][4]."""
    e = np.asarray(e, dtype=np.int64)
    px, c = np.divmod(e, C)
    if cp > 0:
        return px * cp + c
    kw = -cp
    shape = (kw, (kw + 1) // 2, 2, 4)  # per output channel
    co, tap = np.divmod(px, kw * kw)
    kh, kx = np.divmod(tap, kw)
    idx = (kh, kx // 2, kx % 2, c)
    flat = np.zeros_like(e)
    for i, d in zip(idx, shape):
        assert np.all((i >= 0) & (i < d))
        flat = flat * d + i
    return co * int(np.prod(shape)) + flat


# --------------------------------------------------------------------------- gather + normalise
def gather_samples(order, step: int, B: int):
    """Samples of step ``step``: order[(step * B + b) mod len(order)], in
    Python integers (no wrap at 32 or 64 bits)."""
    n = len(order)
    return [int(order[(int(step) * int(B) + b) % n]) for b in range(B)]


def gather_ref(img, order, labels, step: int, B: int, mean, std):
    """(x64 [B, H, W, C], labels [B]) of the gathered batch: (u / 255 - mean)
    / std per channel in fp64, mean / std being the fp32 constants the kernel
    is given."""
    smp = gather_samples(order, step, B)
    u = np.asarray(img)[smp].astype(F64)
    mean64 = np.asarray(mean, dtype=F32).astype(F64)
    std64 = np.asarray(std, dtype=F32).astype(F64)
    return (u / 255.0 - mean64) / std64, np.asarray(labels)[smp]


def gather_error_bound(x64, mean, std):
    """E with |fp32 evaluation - x| <= E for x = (u/255 - mean)/std evaluated
    as (u * r - mean) * q in fp32, r = fp32(1/255), q = fp32(1/std), contracted
    into an fma or not.  With h = 2^-24 (half an ulp, relative) and t = u/255:

    * r carries h, the product u * r another h: |t1 - t| <= 2 h t;
    * the difference d = fl(t1 - mean) adds h |d|: |d - (t - mean)| <= 2 h t + h |t - mean|
      (a contracted fma drops one of the two, never adds);
    * q carries h and the final product h: two more relative h on x.

    Divided by std: E <= h (2 t / std + 3 |x|), and t / std <= |x| + mean / std,
    so E <= h (5 |x| + 2 mean/std) <= 7 h max(|x|, mean/std); 8 h covers the
    second-order terms.  Nothing here is measured from the kernel."""
    ms = np.abs(np.asarray(mean, dtype=F32).astype(F64) / np.asarray(std, dtype=F32).astype(F64))
    return 8.0 * 2.0 ** -24 * np.maximum(np.abs(np.asarray(x64, F64)), ms)


def gather_allowed(x64, mean, std):
    """(lo, hi, exempt): the bf16 values (as fp64) a correct kernel may store
    for x64: bf16(x64) itself -- lo == hi -- unless x64 lies within E of a
    bf16 rounding boundary, where the neighbour on the other side is allowed
    too (rounding is monotonic, so these are bf16(x - E) and bf16(x + E))."""
    E = gather_error_bound(x64, mean, std)
    lo, hi = bf16_round64(x64 - E), bf16_round64(x64 + E)
    return lo, hi, lo != hi


# --------------------------------------------------------------------------- the case matrix shared by the tests
INPLACE_SPLITS = [1, 2, 4, 5, 7, 8, 9, 15, 16, 17, 24, 25, 31]  # 1 lane below 8, else 8; chunk edges; the maximum
TAIL_SPLITS = [1, 4, 5, 7, 8, 25, 31, 32, 33, 40, 127, 128, 129]  # 1 / 8 / 32 lanes, batches of 4 per lane
# (Cout, taps, Cp, C): channel-padded (Cp > 0) and pair-packed (Cp = -KW) tails
TAIL_GEOMS = [(1, 1, 8, 4), (8, 25, 8, 3), (4, 25, -5, 3), (8, 9, -3, 4), (8, 16, -4, 2), (128, 25, 16, 12)]
