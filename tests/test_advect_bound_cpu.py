"""The machinery of tests/advect_bound.py checked without a GPU, against the C oracle alone (which tests/test_oracle.py holds to
the compiled reference bit for bit): the oracle lies within the exact-mode bound of the fp64 value at every decided voxel of
every scene the GPU test uses; few voxels are undecided; and the fast-mode bound is sharp enough to catch a numpy emulation
of the tolerance-mode kernel with one deliberate defect. Run with -s to see the shares and the bound's tightness."""
import numpy as np
import pytest

import advect_bound as A

UNDECIDED_CAP = 0.005          # of the fluid voxels, per scene and operator


@pytest.mark.parametrize("name", A.SCENES)
def test_oracle_within_the_exact_bound_and_few_voxels_undecided(oracle, name):
    sc = A.scene(name)
    for op, method in A.CASES:
        res = A.evaluate(oracle, sc, op, method, "exact")
        got = res["oracle"]
        bad, witness = A.check(got, res)
        fl = A.fluid_voxels(sc["flags"], got)
        share = float((~res["decided"] & fl).sum()) / max(int(fl.sum()), 1)
        sel = res["decided"] & fl & (res["bound"] > 0)
        if op == "advectVel":
            src = np.abs(sc["U"].astype(np.float64))
        else:
            src = np.abs(sc["density"].astype(np.float64))
        # the local magnitude: the largest |input| over the 3^3 neighbourhood (a superset of the box's corners)
        loc = src.copy()
        for ax in (-3, -2, -1):
            loc = np.maximum(loc, np.maximum(np.roll(loc, 1, ax), np.roll(loc, -1, ax)))
        tight = float(np.median(res["bound"][sel] / (A.U32 * np.maximum(loc[sel], 1e-300)))) if sel.any() else 0.0
        print("%-22s %-12s %-14s undecided %.4f%% of fluid voxels, lanes %.1f%%, median bound %.1f u x local magnitude, "
              "oracle err / bound at most %.3f" % (name, op, method, 100 * share, 100.0 * float((res["lanes"] & fl).sum()) / max(int(fl.sum()), 1),
                                                   tight, witness))
        assert not bad.any(), (name, op, method, A.describe(got, res, bad))
        assert share <= UNDECIDED_CAP, (name, op, method, share)
        # where the bound is 0 the value IS the oracle's
        z = res["decided"] & (res["bound"] == 0)
        assert np.array_equal(got[z].astype(np.float64), res["value"][z])


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_fast_vel_euler(sc, oracle_out, defect=None):
    """advectVel eulerOurs as k_vel3_fwd<true> evaluates its lanes, in numpy fp32 (fma through float64); every other voxel takes
    the oracle's value. defect: None, "swap-t" (t and 1 - t swapped on the x axis), "plane" (the z + 1 plane read for z in the
    second row of every 64 x 4 tile)."""
    U, flags, dt = sc["U"], sc["flags"], sc["dt"]
    out = oracle_out.copy()
    for b in range(U.shape[0]):
        f = flags[b, 0]
        plain, inner = f == 1.0, A._inner(f.shape)
        ctr = [c.astype(np.float32) for c in A.centres(f.shape)]
        Z, Y, X = f.shape
        for c in range(3):
            u32 = A.mac_velocity(U[b], c)[0]
            d = [v * np.float32(-dt) for v in u32]
            l2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            nz = l2 > np.float32(1e-6)
            p = [np.where(nz, ctr[a] + d[a], ctr[a]) for a in range(3)]
            lane = inner & plain & (l2 <= A.LEN2_FAST)
            pc = [np.where(lane, p[a], ctr[a]) for a in range(3)]
            lane &= plain[pc[2].astype(np.int64), pc[1].astype(np.int64), pc[0].astype(np.int64)]
            px = [v - np.float32(0.5) for v in pc]
            idx = [np.clip(np.floor(v).astype(np.int64), 0, n - 2) for v, n in zip(px, (X, Y, Z))]     # (clipped off the lanes only)
            t = [(v - np.floor(v)).astype(np.float32) for v in px]
            if defect == "swap-t":
                t[0] = np.float32(1.0) - t[0]
            zi = idx[2].copy()
            if defect == "plane":
                row = (np.arange(Y) % 4 == 1)[None, :, None]
                zi = np.where(row, np.minimum(zi + 1, Z - 2), zi)
            g = A._gather(U[b, c], zi, idx[1], idx[0])
            y = [_fma(t[1], g[n + 2] - g[n], g[n]) for n in (0, 1, 4, 5)]
            x = [_fma(t[0], y[1] - y[0], y[0]), _fma(t[0], y[3] - y[2], y[2])]
            v = _fma(t[2], x[1] - x[0], x[0])
            out[b, c] = np.where(lane, v, out[b, c])
    return out


@pytest.mark.parametrize("name", ["slow-7x13x70", "rough-9x22x129", "small-half-33x16x64"])
def test_the_fast_bound_catches_deliberate_defects(oracle, name):
    sc = A.scene(name)
    res = A.evaluate(oracle, sc, "advectVel", "eulerOurs", "fast")
    ok = emulate_fast_vel_euler(sc, res["oracle"])
    bad, witness = A.check(ok, res)
    print("%s: emulated fast mode, err / bound at most %.3f" % (name, witness))
    assert not bad.any(), A.describe(ok, res, bad)
    assert (ok != res["oracle"])[res["lanes"]].any(), "the emulation never left the exact mode's bits"
    for defect in ("swap-t", "plane"):
        got = emulate_fast_vel_euler(sc, res["oracle"], defect)
        bad, _ = A.check(got, res)
        print("%s: defect %s violates the bound at %d decided voxels" % (name, defect, int(bad.sum())))
        assert bad.any(), defect
    # the correction applied with `strength` instead of `strength / 2` (on the oracle's own forward and backward fields, where
    # the clamp did not act), against the exact-mode bound of maccormackOurs
    for op, fld in (("advectVel", "U"), ("advectScalar", "density")):
        resm = A.evaluate(oracle, sc, op, "maccormackOurs", "exact")
        src = sc[fld].copy()
        if op == "advectVel":
            aux = oracle.advectVel(sc["dt"], src, sc["flags"], "maccormackOurs", None, A.STRENGTH)
        else:
            aux = oracle.advectScalar(sc["dt"], src, sc["U"], sc["flags"], "maccormackOurs", None, False, A.STRENGTH)
        f, bw, orig = aux["fwd"], aux["bwd"], sc[fld]
        hs = float(np.float32(A.STRENGTH)) * 0.5
        diff = (orig - bw).astype(np.float64)
        r1 = (f.astype(np.float64) + hs * diff).astype(np.float32)
        r2 = (f.astype(np.float64) + 2 * hs * diff).astype(np.float32)
        plainly = (r1 == resm["oracle"]) & (r1 != f)
        bad0, _ = A.check(np.where(plainly, r1, resm["oracle"]), resm)
        assert not bad0.any()
        bad, _ = A.check(np.where(plainly, r2, resm["oracle"]), resm)
        print("%s: %s with the whole strength violates the bound at %d decided voxels" % (name, op, int(bad.sum())))
        assert bad.any(), op
