"""Plain reference of the affine angle map (include/qmle_sv.h, qmle_build_angles): NumPy and Python integers only.

    table[b][s] = const[s] + sum_t coef[t] * leaf_{arg[t]}[row_k(b)][idx[t]],  t in [ptr[s], ptr[s + 1]),
    row_k(b)    = ((b + offset) // div_k) % mod_k

Rows come from Python integers (no width to overflow).  The sum runs in float64 in term order; a float32 x float32
product is exact in float64 (24 + 24 <= 53 bits), so `acc + coef * leaf` rounds once, like the kernels' fma, and the sum
equals theirs bit for bit.  Where period[s] > 0 and the sum lies beyond +-period it is reduced as
acc - per * rint(acc / per); then everything is cast to float32.  The kernels' compiler may fuse that last multiply and
subtract: `reduce_fused` is that form (exact product, one rounding), `reduce_unfused` the written one.

Also here: hand-built maps (`identity_map`, `affine_map`) as host arrays, and their upload into an
`_native.AngleMapArgs` (`MapArrays.device`)."""
from fractions import Fraction

import numpy as np

FOUR_PI = 4.0 * np.pi


def reduce_unfused(acc: float, per: float) -> float:
    """acc - per * rint(acc / per), every operation rounded to float64 (the expression as the kernels write it)."""
    acc, per = np.float64(acc), np.float64(per)
    return float(acc - per * np.rint(acc / per))


def reduce_fused(acc: float, per: float) -> float:
    """fma(-per, rint(acc / per), acc): the product exact, one rounding at the end (rational arithmetic; the
    conversion of a Fraction to float rounds correctly)."""
    k = float(np.rint(np.float64(acc) / np.float64(per)))
    return float(Fraction(acc) - Fraction(per) * Fraction(k))


def row_of(b: int, offset: int, div: int, mod: int) -> int:
    return ((int(b) + int(offset)) // int(div)) % int(mod)


def sums(leaves, strides, divs, mods, ptr, arg, idx, coef, const, batch, offset):
    """The float64 sums before any reduction, [batch, n_slots].  leaves[k]: float32 array (flattened per row with
    `strides[k]` floats per row) or None for a leaf no term refers to."""
    n_slots = len(ptr) - 1
    flat = [None if l is None else np.asarray(l, dtype=np.float32).reshape(-1) for l in leaves]
    coef32, const32 = np.asarray(coef, dtype=np.float32), np.asarray(const, dtype=np.float32)
    out = np.zeros((batch, n_slots), dtype=np.float64)
    for b in range(batch):
        row = [row_of(b, offset, divs[k], mods[k]) for k in range(len(leaves))]
        for s in range(n_slots):
            acc = np.float64(const32[s])
            for t in range(int(ptr[s]), int(ptr[s + 1])):
                k = int(arg[t])
                leaf = flat[k][row[k] * int(strides[k]) + int(idx[t])]
                acc = acc + np.float64(coef32[t]) * np.float64(leaf)  # exact product, one rounding: an fma
            out[b, s] = acc
    return out


def table(leaves, strides, divs, mods, ptr, arg, idx, coef, const, period, batch, offset):
    """-> (float32 table [batch, n_slots], bool mask of the entries that were reduced).  period: one double per slot or
    None (no slot is periodic)."""
    acc = sums(leaves, strides, divs, mods, ptr, arg, idx, coef, const, batch, offset)
    per = np.zeros(acc.shape[1]) if period is None else np.asarray(period, dtype=np.float64)
    per = np.broadcast_to(per[None, :acc.shape[1]], acc.shape)
    mask = (per > 0.0) & ((acc > per) | (acc < -per))
    red = acc.copy()
    red[mask] = acc[mask] - per[mask] * np.rint(acc[mask] / per[mask])
    return red.astype(np.float32), mask


def ulp_distance(a, b):
    """Distance of float32 arrays in units in the last place (ordered-integer view; +0 and -0 coincide)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    return np.abs(key(a) - key(b))


def mod_distance(a, b, per=FOUR_PI):
    """|a - b| modulo `per` in float64: how far two angles are as arguments of a `per`-periodic gate."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return np.abs(d - per * np.rint(d / per))


class MapArrays:
    """One affine map as host arrays: ptr / arg / idx int32, coef / const float32, period float64 or None."""

    def __init__(self, ptr, arg, idx, coef, const, period=None):
        self.ptr, self.arg, self.idx = (np.asarray(v, dtype=np.int32) for v in (ptr, arg, idx))
        self.coef, self.const = np.asarray(coef, dtype=np.float32), np.asarray(const, dtype=np.float32)
        self.period = None if period is None else np.asarray(period, dtype=np.float64)
        self.n_slots = len(self.ptr) - 1
        assert len(self.const) == self.n_slots and self.ptr[-1] == len(self.arg) == len(self.idx) == len(self.coef)
        self._dev = None

    def table(self, leaves, strides, divs, mods, batch, offset=0):
        return table(leaves, strides, divs, mods, self.ptr, self.arg, self.idx, self.coef, self.const, self.period,
                     batch, offset)

    def device(self):
        """(d_ptr, d_arg, d_idx, d_coef, d_const, d_period or None) on the current GPU, uploaded once."""
        if self._dev is None:
            import torch

            pad = lambda v: v if len(v) else np.zeros(1, dtype=v.dtype)  # (an empty tensor has no address)
            self._dev = tuple(None if v is None else torch.from_numpy(pad(v)).cuda()
                              for v in (self.ptr, self.arg, self.idx, self.coef, self.const, self.period))
        return self._dev

    def args(self, n_leaves):
        """A fresh `_native.AngleMapArgs` of this map (set its leaves per call)."""
        from qml_essentials_amd import _native as N

        return N.AngleMapArgs(n_leaves, *self.device())


def identity_map(n_slots, period=None):
    """Slot s = column s of leaf 0."""
    return MapArrays(np.arange(n_slots + 1), np.zeros(n_slots), np.arange(n_slots), np.ones(n_slots),
                     np.zeros(n_slots), period)


def affine_map(n_slots, widths, rng, period=None, big=(), max_terms=3, coef_scale=1.0):
    """Several terms per slot, leaves shared between slots, constants: slot s takes 1..max_terms terms over the leaves
    of `widths` floats per row (every slot's first term is on leaf s % n_leaves, so every leaf is used), coefficients
    uniform in +-coef_scale; the slots of `big` get one coefficient of 3^7 on top (sums of ~1e4 rad for leaves of a few
    radians)."""
    ptr, arg, idx, coef, const = [0], [], [], [], []
    for s in range(n_slots):
        for j in range(int(rng.integers(1, max_terms + 1))):
            k = s % len(widths) if j == 0 else int(rng.integers(len(widths)))
            arg.append(k)
            idx.append(int(rng.integers(widths[k])))
            coef.append(float(rng.uniform(-coef_scale, coef_scale)))
        if s in big:
            coef[-1] = float(3 ** 7) * (1.0 if rng.random() < 0.5 else -1.0)
        const.append(float(rng.uniform(-1.0, 1.0)))
        ptr.append(len(arg))
    return MapArrays(ptr, arg, idx, coef, const, period)
