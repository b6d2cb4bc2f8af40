"""Helper of tests/test_divnorm_cpu.py and tests/test_hip_divnorm.py: the cases of the divergence-norm operator
(tfl_velocityDivergenceNorm), its expected value and the bound the device result is held to.

Expected value: the fp32 divergence of the CPU checker's velocityDivergenceForward (the device divergence is bit-equal to it:
tests/test_hip_parity.py), converted to float64, squared (exact: an fp32 square fits 48 bits), summed with math.fsum (exact,
rounded once) and rooted. Bound: a sum of N non-negative doubles in any order has relative error at most (N - 1) 2^-53 to
first order, and the root adds one rounding, so |norm - exact| <= (N + 2) 2^-53 exact with N = Z Y X. Derived, not measured."""
import math

import numpy as np

import scenes

# (name, dims (Z, Y, X), B, how the device tensors are laid out)
CASES = [
    ("3d-16x24x32", (16, 24, 32), 1, "aligned"),
    ("3d-32x32x32-b2", (32, 32, 32), 2, "aligned"),
    ("3d-ragged-13x17x23", (13, 17, 23), 1, "aligned"),          # X % 4 != 0: the one-cell-per-thread form
    ("3d-ragged-b2", (13, 17, 23), 2, "aligned"),
    ("3d-short-row-8x12x16", (8, 12, 16), 2, "aligned"),         # a row far narrower than 128 cells: 8-lane row segments
    ("3d-wide-row-6x10x160", (6, 10, 160), 1, "aligned"),        # a row wider than one 32-lane segment: the memory tap at its end
    ("2d-64x96", (1, 64, 96), 1, "aligned"),
    ("2d-64x96-b2", (1, 64, 96), 2, "aligned"),
    ("2d-ragged-33x47", (1, 33, 47), 2, "aligned"),
    ("3d-misaligned-view", (16, 24, 32), 1, "misaligned"),       # sliced one element off a 16-byte boundary
    ("2d-misaligned-view", (1, 64, 96), 2, "misaligned"),
]
MIN_EXACT = 1e-3      # every sample of every case: the comparison must not pass on nothing


def make_case(name):
    """(U, flags) as numpy arrays for the case `name`: random smooth velocities of 0.4 cells per step, obstacles"""
    for i, (n, dims, B, _) in enumerate(CASES):
        if n == name:
            sc = scenes.make_scene(dims, seed=40 + i, B=B, vel_cells=0.4)
            return sc["U"], sc["flags"]
    raise KeyError(name)


def exact_norm(oracle, U, flags):
    """[B] float64: the divergence norm of each sample, exactly summed"""
    div = np.zeros_like(flags)
    oracle.velocityDivergenceForward(np.ascontiguousarray(U), np.ascontiguousarray(flags), div)
    out = []
    for b in range(div.shape[0]):
        d = div[b].astype(np.float64).ravel()
        out.append(math.sqrt(math.fsum(d * d)))
    return np.array(out, np.float64)


def bound(dims, exact):
    """the largest |norm - exact| the reduction may show, per sample"""
    Z, Y, X = dims
    return (Z * Y * X + 2) * 2.0 ** -53 * exact
