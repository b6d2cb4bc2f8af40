"""Per-voxel fp64 error bounds for the trace-based advection operators (advectVel, advectScalar; eulerOurs, maccormackOurs;
3-D), in the exact and in the tolerance mode of the LDS-tiled kernels (advect_vel3_kernels.hpp, advect_scalar3.hip, advect_pair3.hip).

advect_vel() / advect_scalar() evaluate the operator in float64 from its definition on the same fp32 inputs and give, beside
every value, an upper bound on how far an fp32 evaluation in the named arithmetic (`mode`) may lie from it -- running-error
analysis in the style of tests/conv_bound.py, all in fp64, u = 2^-24, gamma(n) = n u / (1 - n u). No constant is fitted.

Which arithmetic a voxel sees.  A LANE is a voxel the kernels keep on their straight-line path (trace_fast() returns true):
not a border cell, a fluid cell (advectVel: the plain word 1.0), displacement no longer than 0.99 cell, end point in a fluid
(plain fluid) cell. Every other voxel runs the generic functions of tfl_device.hpp, which are the exact-mode code in BOTH
modes: there the value is the oracle's own and the bound is 0 (the GPU must give those bits), except in pass B of
maccormackOurs, where a generic voxel still interpolates forward-field values that lanes wrote (below).

Discrete decisions that do not depend on the trace arithmetic are taken as the kernels take them, in fp32 (numpy float32 is
IEEE single): the MAC average, d = u * dt, |d|^2 > 1e-6, the hand-over tests, the clamp box int(pos -+ vel). Decisions that DO
depend on it (which cell the end point lies in: the fluid test, the interpolation box and its dropped taps, the 3^3 clamp
neighbourhood of the scalar) are taken from the fp64 end point, and a voxel whose end point lies within the position bound
`delta` of a cell face or of a cell-centre plane (where the interpolation box changes) is UNDECIDED: no statement is made
there, nor at a pass-B voxel that reads an undecided forward value.

The error terms (kernel lines in brackets):
  u        MAC average 0.25f * (((a + b) + c) + d) [mac_from_tile]: three additions, the scaling exact: gamma(3) (|a| + .. + |d|)
           / 4; the component's own face is read, not averaged: 0. Scalar: 0.5f * (a + b) [centred]: u (|a| + |b|) / 2.
  d        d = u * dt [trace_fast, scale3]: |dt| e_u + u |d|.
  p exact  q = d / len, p = ctr + q * len [trace_fast / line_trace]: the quotient and the product round once each and the
           error of len cancels between them (q len = d (1 + d1)(1 + d2)): gamma(2) |d|; the addition: u |p|.
  p fast   p = ctr + d: the addition, u |p|.
  sample   position error times the local slope: sum over the axes of delta_a * (largest difference along a of the box's
           four edges) -- the derivative of a trilinear form along an axis is a convex combination of those differences; with
           dropped taps (getInterpolatedWithFluidHi) the form is the plain one on the box with every missing corner replaced
           by its partner of the same 1-D lerp, y first, then x, then z [lerp_fluid / lerp1_fluid].
           p - 0.5 and the fraction are exact (both operands are multiples of ulp(p)); 1 - t rounds once.
  exact    (g000 t0 + g010 t1) s0 + .. [lerp8<false>, interpol]: a corner's product passes 6 operations and up to 3 rounded
           weights (t0, s0, f0): gamma(9) sum |w_i| |g_i|.
  fast     seven a + t (b - a) [lerp8<true>, lerp1<true>]: the subtraction and the fma round once each: per lerp
           u t |b - a| + u |result|, carried through the three levels as a running error (gamma x sum |w g| does not bound this
           form: t |b - a| may exceed the weighted magnitudes).
  pass B   the forward field's own bound enters through the box's corners (their largest: the weights sum to 1) and through
           the voxel's own forward value.
  correct  f + strength/2 (orig - bwd): orig - bwd is an fp32 subtraction in BOTH modes (one rounding); then exact mode
           evaluates in double and rounds once to fp32 [tfluids.cc:231/:693], fast mode one fma (one rounding). (float)
           half_strength is exact: strength is an fp32 number and halving it is exact. So both modes: |hs| u |orig - bwd| +
           u |result| (+ 4 x 2^-53 of the magnitudes for the double operations).
  clamp    1-Lipschitz; its limits are extrema of inputs: exact.
"""
import ctypes

import numpy as np

U32 = 2.0 ** -24
FLUID = 1
LEN_FAST = np.float32(0.99)                      # kFastLen
LEN2_FAST = np.float32(0.99) * np.float32(0.99)  # kFastLen * kFastLen, an fp32 product (constant-folded the same way)


def gamma(n, r=U32):
    return n * r / (1.0 - n * r)


def _sh(A, dz, dy, dx):
    """A at (k + dz, j + dy, i + dx) (wraps at the array's faces: only non-border cells are used)"""
    return np.roll(A, (-dz, -dy, -dx), (-3, -2, -1))


_E = ((0, 0, 1), (0, 1, 0), (1, 0, 0))         # unit offsets (dz, dy, dx) of the axes x, y, z


def _neg(e):
    return tuple(-v for v in e)


def _add(a, b):
    return tuple(x + y for x, y in zip(a, b))


def mac_velocity(U, c):
    """get_at_mac of face c: (u32[3], u64[3], e_u[3]), every entry [Z, Y, X]"""
    u32, u64, eu = [], [], []
    for a in range(3):
        if a == c:
            u32.append(U[a].copy()); u64.append(U[a].astype(np.float64)); eu.append(np.zeros(U[a].shape))
            continue
        offs = ((0, 0, 0), _neg(_E[c]), _E[a], _add(_neg(_E[c]), _E[a]))
        t = [_sh(U[a], *o) for o in offs]
        u32.append(np.float32(0.25) * (((t[0] + t[1]) + t[2]) + t[3]))
        t64 = [v.astype(np.float64) for v in t]
        u64.append(0.25 * (t64[0] + t64[1] + t64[2] + t64[3]))
        eu.append(gamma(3) * 0.25 * sum(np.abs(v) for v in t64))
    return u32, u64, eu


def centred_velocity(U):
    """get_centered: 0.5f * (U[a] + U[a + e_a])"""
    u32, u64, eu = [], [], []
    for a in range(3):
        p, q = U[a], _sh(U[a], *_E[a])
        u32.append(np.float32(0.5) * (p + q))
        u64.append(0.5 * (p.astype(np.float64) + q.astype(np.float64)))
        eu.append(U32 * 0.5 * (np.abs(p.astype(np.float64)) + np.abs(q.astype(np.float64))))
    return u32, u64, eu


def centres(shape):
    Z, Y, X = shape
    k, j, i = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return [i + 0.5, j + 0.5, k + 0.5]          # x, y, z


class Trace:
    """one back-trace per voxel of the displacement u * ndt from the cell centres"""

    def __init__(self, u32, u64, eu, ndt, mode):
        ndt32 = np.float32(ndt)
        d32 = [v * ndt32 for v in u32]
        self.d32 = d32
        self.l2 = (d32[0] * d32[0] + d32[1] * d32[1]) + d32[2] * d32[2]       # fp32, the kernels' association
        self.nz = self.l2 > np.float32(1e-6)
        adt = abs(float(ndt32))
        ctr = centres(u32[0].shape)
        self.p, self.delta = [], []
        for a in range(3):
            d64 = np.where(self.nz, u64[a] * float(ndt32), 0.0)
            ed = np.where(self.nz, adt * eu[a] + U32 * (np.abs(d64) + adt * eu[a]), 0.0)
            p = ctr[a] + d64
            if mode == "fast":
                dl = ed + U32 / (1 - U32) * (np.abs(p) + ed)
            else:
                q = ed + gamma(2) * (np.abs(d64) + ed)
                dl = q + U32 / (1 - U32) * (np.abs(p) + q)
            self.p.append(p)
            self.delta.append(np.where(self.nz, dl, 0.0))
        with np.errstate(invalid="ignore"):
            self.short_exact = np.sqrt(self.l2) <= LEN_FAST                 # len <= 0.99f (sqrtf is correctly rounded)
            self.short_fast = self.l2 <= LEN2_FAST
        # |d| within the rounding of either hand-over test (l2 carries gamma(3), the root u more: 8 u of 0.99^2 covers both)
        self.handover = np.abs(self.l2.astype(np.float64) - float(LEN2_FAST)) <= 8 * U32
        # the end point within delta of a cell face (integer) or of a centre plane (half-integer)
        near = np.zeros(self.l2.shape, bool)
        for a in range(3):
            t = self.p[a] * 2.0
            near |= np.abs(t - np.rint(t)) <= 2.0 * self.delta[a]
        self.near = near & self.nz


def _gather(g, zi, yi, xi):
    return [g[zi + dz, yi + dy, xi + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]      # n = 4 dz + 2 dy + dx


def box_of(P, shape):
    """buildIndex: cell and fractions of the interpolation box of P = (x, y, z)"""
    Z, Y, X = shape
    out = []
    for p, n in zip(P, (X, Y, Z)):
        pc = np.clip(p - 0.5, 0.0, n - 1.0)
        idx = np.minimum(np.floor(pc).astype(np.int64), n - 2)
        out.append((idx, pc - idx))
    return out


def _fill(c, e, m):
    """replace every dropped corner by what lerp_fluid uses in its place (y pairs, then x, then z); False where no corner is fluid"""
    c, e, m = [v.copy() for v in c], [v.copy() for v in e], [v.copy() for v in m]

    def merge(ga, gb):
        va = np.zeros(c[0].shape, bool)
        vb = np.zeros(c[0].shape, bool)
        for n in ga:
            va |= m[n]
        for n in gb:
            vb |= m[n]
        for na, nb in zip(ga, gb):
            ta, tb = ~va & vb, va & ~vb
            c[na] = np.where(ta, c[nb], c[na]); e[na] = np.where(ta, e[nb], e[na])
            c[nb] = np.where(tb, c[na], c[nb]); e[nb] = np.where(tb, e[na], e[nb])
        for n in ga + gb:
            m[n] = va | vb
    for dz in (0, 1):
        for dx in (0, 1):
            merge([4 * dz + dx], [4 * dz + 2 + dx])
    for dz in (0, 1):
        merge([4 * dz, 4 * dz + 2], [4 * dz + 1, 4 * dz + 3])
    merge([0, 1, 2, 3], [4, 5, 6, 7])
    return c, e, m[0]


def sample(g, ge, P, delta, form, fluid=None):
    """(value, bound) of the trilinear sample of g (fp64, each entry within ge of what the kernel reads) at P, whose fp32
    counterpart lies within delta (per axis) of it, in the interpolation `form` ("exact" / "fast", or a boolean array: True =
    fast); fluid: the mask of getInterpolatedWithFluidHi (None: plain interpol)."""
    (xi, tx), (yi, ty), (zi, tz) = box_of(P, g.shape)
    c, e = _gather(g, zi, yi, xi), _gather(ge, zi, yi, xi)
    if fluid is not None:
        m = _gather(fluid, zi, yi, xi)
        cf, ef, ok = _fill(c, e, m)
        c = [np.where(ok, a, b) for a, b in zip(cf, c)]          # no fluid corner at all: the plain sample (grid.cc:328)
        e = [np.where(ok, a, b) for a, b in zip(ef, e)]
    emax = np.max(e, axis=0)
    M = np.max(np.abs(c), axis=0) + emax
    # slopes: the largest edge difference along each axis (+ 2 emax: the kernel's corners are within e of these)
    sx = np.max([np.abs(c[n + 1] - c[n]) for n in (0, 2, 4, 6)], axis=0) + 2 * emax
    sy = np.max([np.abs(c[n + 2] - c[n]) for n in (0, 1, 4, 5)], axis=0) + 2 * emax
    sz = np.max([np.abs(c[n + 4] - c[n]) for n in (0, 1, 2, 3)], axis=0) + 2 * emax
    pos = delta[0] * sx + delta[1] * sy + delta[2] * sz
    dsum = delta[0] + delta[1] + delta[2]

    def lerp(a, b, t):
        return a + t * (b - a)
    y = [lerp(c[n], c[n + 2], ty) for n in (0, 1, 4, 5)]         # (dz, dx) = 00, 01, 10, 11
    x = [lerp(y[0], y[1], tx), lerp(y[2], y[3], tx)]
    val = lerp(x[0], x[1], tz)
    # exact form: gamma(9) sum |w| (|g| + e), the weights' shift by delta adding at most 2 M per axis
    ay = [lerp(np.abs(c[n]) + e[n], np.abs(c[n + 2]) + e[n + 2], ty) for n in (0, 1, 4, 5)]
    ax = [lerp(ay[0], ay[1], tx), lerp(ay[2], ay[3], tx)]
    mag = lerp(ax[0], ax[1], tz) + 2 * M * dsum
    r_exact = gamma(9) * mag

    # fast form: running error of r = fma(t, b - a, a): u t (|b - a| + ea + eb) for the subtraction, u (|r| + all before) for the fma
    def lerp_e(a, ea, b, eb, t):
        r = lerp(a, b, t)
        e0 = lerp(ea, eb, t)
        e1 = U32 * t * (np.abs(b - a) + ea + eb)
        return r, e0 + e1 + U32 * (np.abs(r) + e0 + e1)
    zero = np.zeros(val.shape)
    fy = [lerp_e(c[n], zero, c[n + 2], zero, ty) for n in (0, 1, 4, 5)]
    fx = [lerp_e(*fy[0], *fy[1], tx), lerp_e(*fy[2], *fy[3], tx)]
    # (the corners' own errors: 3 u each per lerp over the 3 levels of a path; the weights' shift by delta: at most 2 M per axis and lerp)
    r_fast = lerp_e(*fx[0], *fx[1], tz)[1] + 9 * U32 * emax + 7 * U32 * 2 * M * dsum
    if isinstance(form, str):
        rnd = r_fast if form == "fast" else r_exact
    else:
        rnd = np.where(form, r_fast, r_exact)
    return val, emax + pos + rnd


def _trace_generic(oracle, flags3, d32, need):
    """end points of the reference's line trace from the centres of the voxels `need` with displacement d32 (fp32, what both modes
    compute off the lanes); other voxels get their centre"""
    shape = flags3.shape
    ctr = centres(shape)
    P = [c.astype(np.float64).copy() for c in ctr]
    idx = np.flatnonzero(need)
    if idx.size == 0:
        return P
    pos = np.stack([ctr[a].reshape(-1)[idx] for a in range(3)], 1).astype(np.float32)
    dl = np.stack([d32[a].reshape(-1)[idx] for a in range(3)], 1).astype(np.float32)
    out = np.zeros_like(pos)
    f = np.ascontiguousarray(flags3, np.float32)
    fn = oracle.lib.ora_calcLineTrace
    pb, db, ob, fp = pos.ctypes.data, dl.ctypes.data, out.ctypes.data, ctypes.c_void_p(f.ctypes.data)
    Z, Y, X = shape
    vp = ctypes.c_void_p
    for n in range(idx.size):
        fn(vp(pb + 12 * n), vp(db + 12 * n), fp, Z, Y, X, 1, vp(ob + 12 * n))
    for a in range(3):
        P[a].reshape(-1)[idx] = out[:, a]
    return P


def _cell_ok(cellmask, P):
    Z, Y, X = cellmask.shape
    xi = np.clip(np.floor(P[0]).astype(np.int64), 0, X - 1)
    yi = np.clip(np.floor(P[1]).astype(np.int64), 0, Y - 1)
    zi = np.clip(np.floor(P[2]).astype(np.int64), 0, Z - 1)
    return cellmask[zi, yi, xi]


def _inner(shape):
    m = np.zeros(shape, bool)
    m[1:-1, 1:-1, 1:-1] = True
    return m


def _correct(f, ef, orig, bw, ebw, hs):
    """(value, bound) of f + hs (orig - bwd), see `correct` in the module comment"""
    diff = orig - bw
    r = f + hs * diff
    e0 = ef + abs(hs) * ebw
    e1 = abs(hs) * U32 * (np.abs(diff) + ebw)
    dbl = 4 * 2.0 ** -53 * (np.abs(f) + ef + abs(hs) * (np.abs(diff) + ebw))
    return r, e0 + e1 + dbl + U32 * (np.abs(r) + e0 + e1 + dbl)


def _item_vel(oracle, dt, U, flags, method, strength, mode, ofwd, oout):
    """one batch item: U [3, Z, Y, X], flags [Z, Y, X]; ofwd / oout: the oracle's forward field and result"""
    shape = flags.shape
    fi = flags.astype(np.int64)
    fluid = (fi & FLUID) != 0
    plain = flags == 1.0
    inner = _inner(shape)
    mac = method == "maccormackOurs"
    hs = float(np.float32(strength)) * 0.5
    value = oout.astype(np.float64).copy()
    bound = np.zeros(value.shape)
    decided = np.ones(value.shape, bool)
    lanes = np.zeros(value.shape, bool)
    fwd64 = ofwd.astype(np.float64).copy() if mac else None
    eA = np.zeros(value.shape)
    badA = np.zeros(value.shape, bool)
    zero3 = np.zeros(shape)
    keep = {}
    for c in range(3):
        u32, u64, eu = mac_velocity(U, c)
        tA = Trace(u32, u64, eu, -dt, mode)
        short = (tA.short_fast | tA.handover) if mode == "fast" else tA.short_exact
        cand = inner & plain & short
        L = cand & ~tA.near & _cell_ok(plain, tA.p)
        und = cand & tA.near
        v, e = sample(U[c].astype(np.float64), zero3, tA.p, tA.delta, mode)
        ref = (ofwd if mac else oout)[c].astype(np.float64)
        if mode == "fast":       # a lane at the hand-over may have gone either way: the bound then covers the generic result too
            e = e + np.where(tA.handover, np.abs(ref - v), 0.0)
        if mac:
            fwd64[c] = np.where(L, v, fwd64[c]); eA[c] = np.where(L, e, 0.0); badA[c] = und
        else:
            value[c] = np.where(L, v, value[c]); bound[c] = np.where(L, e, 0.0); decided[c] = ~und
            lanes[c] = L
        keep[c] = (u32, u64, eu, tA, cand)
    if not mac:
        return value, bound, decided, lanes
    for c in range(3):
        u32, u64, eu, tA, candA = keep[c]
        tB = Trace(u32, u64, eu, dt, mode)
        cand = candA                                   # the same |d|: the same hand-over
        LB = cand & ~tB.near & _cell_ok(plain, tB.p) & ~(tB.handover if mode == "fast" else False)
        und = cand & (tB.near | (tB.handover if mode == "fast" else False))
        act = inner & fluid                             # the cells whose component c is traced back at all
        gen = act & ~LB & ~und
        Pg = _trace_generic(oracle, flags, tB.d32, gen)
        P = [np.where(LB, tB.p[a], Pg[a]) for a in range(3)]
        dl = [np.where(LB, tB.delta[a], 0.0) for a in range(3)]
        form = LB if mode == "fast" else "exact"
        bw, ebw = sample(fwd64[c], eA[c], P, dl, form)
        # a corner (or the voxel's own forward value) without a statement
        (xi, _), (yi, _), (zi, _) = box_of(P, shape)
        bad = np.any(_gather(badA[c], zi, yi, xi), axis=0) | badA[c]
        emax_corner = np.max(_gather(eA[c], zi, yi, xi), axis=0)
        skip = ~fluid | ~_sh(fluid, *_neg(_E[c]))
        orig = U[c].astype(np.float64)
        r, er = _correct(fwd64[c], eA[c], orig, bw, ebw, hs)
        r = np.where(skip, fwd64[c], r); er = np.where(skip, eA[c], er)
        # MacCormackClampMAC: the box corners of int(pos -+ vel), vel = u * dt in fp32, indices clamped to [0, N - 2]
        Z, Y, X = shape
        ijk = [cc - 0.5 for cc in centres(shape)]
        vel = [v * np.float32(dt) for v in u32]
        lo, hi = np.full(shape, np.inf), np.full(shape, -np.inf)
        with np.errstate(invalid="ignore"):
            for sgn in (-1, 1):
                q = [(ijk[a].astype(np.float32) + np.float32(sgn) * vel[a]) for a in range(3)]
                q = [np.where(np.isfinite(v), v, 0.0) for v in q]
                i0 = np.clip(np.trunc(q[0]).astype(np.int64), 0, X - 2)
                j0 = np.clip(np.trunc(q[1]).astype(np.int64), 0, Y - 2)
                k0 = np.clip(np.trunc(q[2]).astype(np.int64), 0, Z - 2)
                cs = _gather(orig, k0, j0, i0)
                lo = np.minimum(lo, np.min(cs, axis=0)); hi = np.maximum(hi, np.max(cs, axis=0))
        r = np.clip(r, lo, hi)
        # a generic voxel none of whose inputs a lane wrote runs the exact-mode code on the exact-mode bits: the oracle's value
        same = gen & (emax_corner == 0) & (eA[c] == 0) & ~bad
        use = act & ~same
        value[c] = np.where(use, r, value[c])
        bound[c] = np.where(use, er, 0.0)
        decided[c] = ~(act & (und | bad))
        lanes[c] = LB
    return value, bound, decided, lanes


def advect_vel(oracle, dt, U, flags, method, strength=0.75, mode="exact"):
    """dict(value, bound, decided, lanes, oracle): arrays of U's shape. `oracle` = the fp32 result of the reference arithmetic."""
    assert U.shape[1] == 3 and method in ("eulerOurs", "maccormackOurs") and mode in ("exact", "fast")
    out = U.copy()
    aux = oracle.advectVel(dt, out, flags, method, None, strength)
    res = [_item_vel(oracle, dt, U[b], flags[b, 0], method, strength, mode, aux["fwd"][b], out[b]) for b in range(U.shape[0])]
    return dict(value=np.stack([r[0] for r in res]), bound=np.stack([r[1] for r in res]), decided=np.stack([r[2] for r in res]),
                lanes=np.stack([r[3] for r in res]), oracle=out)


def _clamp_bounds_scalar(s64, fluid, P):
    """getClampBounds: extrema of s over the fluid cells inside the grid of the 3^3 neighbourhood of the (clamped) cell of P"""
    Z, Y, X = fluid.shape
    i0 = np.clip(np.trunc(P[0]).astype(np.int64), 0, X - 1)
    j0 = np.clip(np.trunc(P[1]).astype(np.int64), 0, Y - 1)
    k0 = np.clip(np.trunc(P[2]).astype(np.int64), 0, Z - 1)
    lo, hi = np.full(fluid.shape, np.inf), np.full(fluid.shape, -np.inf)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k, j, i = k0 + dz, j0 + dy, i0 + dx
                ok = (k >= 0) & (k < Z) & (j >= 0) & (j < Y) & (i >= 0) & (i < X)
                k, j, i = np.clip(k, 0, Z - 1), np.clip(j, 0, Y - 1), np.clip(i, 0, X - 1)
                ok &= fluid[k, j, i]
                v = s64[k, j, i]
                lo = np.where(ok & (v < lo), v, lo); hi = np.where(ok & (v > hi), v, hi)
    return lo, hi


def _item_scalar(dt, s, U, flags, method, strength, mode, aux, oout):
    shape = flags.shape
    fluid = (flags.astype(np.int64) & FLUID) != 0
    inner = _inner(shape)
    mac = method == "maccormackOurs"
    hs = float(np.float32(strength)) * 0.5
    s64 = s.astype(np.float64)
    zero3 = np.zeros(shape)
    u32, u64, eu = centred_velocity(U)
    tA = Trace(u32, u64, eu, -dt, mode)
    short = (tA.short_fast | tA.handover) if mode == "fast" else tA.short_exact
    cand = inner & fluid & short
    LA = cand & ~tA.near & _cell_ok(fluid, tA.p)
    undA = cand & tA.near
    v, e = sample(s64, zero3, tA.p, tA.delta, mode, fluid)
    ref = (aux["fwd"] if mac else oout).astype(np.float64)
    if mode == "fast":
        e = e + np.where(tA.handover, np.abs(ref - v), 0.0)
    if not mac:
        return np.where(LA, v, ref), np.where(LA, e, 0.0), ~undA, LA
    fwd64, eA = np.where(LA, v, ref), np.where(LA, e, 0.0)
    tB = Trace(u32, u64, eu, dt, mode)
    ho = tB.handover if mode == "fast" else np.zeros(shape, bool)
    LB = cand & ~tB.near & _cell_ok(fluid, tB.p) & ~ho
    undB = cand & (tB.near | ho)
    act = inner & fluid
    gen = act & ~LB & ~undB
    bp = aux["bwdPos"].astype(np.float64)
    P = [np.where(LB, tB.p[a], bp[a]) for a in range(3)]
    dl = [np.where(LB, tB.delta[a], 0.0) for a in range(3)]
    bw, ebw = sample(fwd64, eA, P, dl, LB if mode == "fast" else "exact", fluid)
    (xi, _), (yi, _), (zi, _) = box_of(P, shape)
    bad = np.any(_gather(undA, zi, yi, xi), axis=0) | undA
    emax_corner = np.max(_gather(eA, zi, yi, xi), axis=0)
    r, er = _correct(fwd64, eA, s64, bw, ebw, hs)
    # MacCormackClampOurs around the cell of the FORWARD position (a lane's: from the fp64 end point, decided; else the oracle's)
    fp = aux["fwdPos"].astype(np.float64)
    PA = [np.where(LA, tA.p[a], fp[a]) for a in range(3)]
    lo, hi = _clamp_bounds_scalar(s64, fluid, PA)
    r = np.where(lo > hi, fwd64, np.clip(r, np.minimum(lo, hi), hi))
    er = np.where(lo > hi, eA, er)
    same = gen & (emax_corner == 0) & (eA == 0) & ~bad
    use = act & ~same
    value = np.where(use, r, oout.astype(np.float64))
    return value, np.where(use, er, 0.0), ~(act & (undB | bad)), LB & LA


def advect_scalar(oracle, dt, s, U, flags, method, strength=0.75, mode="exact"):
    assert U.shape[1] == 3 and method in ("eulerOurs", "maccormackOurs") and mode in ("exact", "fast")
    out = s.copy()
    aux = oracle.advectScalar(dt, out, U, flags, method, None, False, strength)
    res = []
    for b in range(U.shape[0]):
        ab = {k: (v[b, 0] if v.shape[1] == 1 else v[b]) for k, v in aux.items()}
        res.append(_item_scalar(dt, s[b, 0], U[b], flags[b, 0], method, strength, mode, ab, out[b, 0]))
    st = lambda n: np.stack([r[n] for r in res])[:, None]
    return dict(value=st(0), bound=st(1), decided=st(2), lanes=st(3), oracle=out)


def fluid_voxels(flags, like):
    """mask of `like`'s shape: non-border fluid cells (every channel)"""
    f = (flags.astype(np.int64) & FLUID) != 0
    f[:, :, [0, -1]] = False; f[:, :, :, [0, -1]] = False; f[..., [0, -1]] = False
    return np.broadcast_to(f, like.shape)


def check(got, res):
    """(violations, witness): the decided voxels where `got` leaves the bound (a bound of 0 asks for the value's bits), and the
    largest error / bound among the decided voxels with a non-zero bound"""
    err = np.abs(got.astype(np.float64) - res["value"])
    bad = res["decided"] & ~(err <= res["bound"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(res["decided"] & (res["bound"] > 0), err / res["bound"], 0.0)
    return bad, float(ratio.max()) if ratio.size else 0.0


def describe(got, res, bad):
    i = np.unravel_index(int(np.argmax(np.where(bad, np.abs(got - res["value"]) / np.maximum(res["bound"], 1e-300), 0))), got.shape)
    return "%d voxels over; worst at %s: got %.9g fp64 %.9g bound %.3g oracle %.9g lane %s" % (
        int(bad.sum()), i, float(got[i]), float(res["value"][i]), float(res["bound"][i]), float(res["oracle"][i]), bool(res["lanes"][i]))


# ---- the scenes of the advection bound tests (tests/test_advect_bound_cpu.py, tests/test_hip_advect_bound.py) -----------------
def _exotic(sc, seed, frac=0.02):
    f = sc["flags"]
    rng = np.random.RandomState(seed)
    fl = np.flatnonzero(f == 1.0)
    pick = rng.choice(fl, size=max(1, int(fl.size * frac)), replace=False)
    f.reshape(-1)[pick] = rng.choice([9.0, 33.0], size=pick.size)
    return sc


def scene(name):
    import scenes
    if name == "slow-7x13x70":
        return scenes.make_scene((7, 13, 70), seed=901, vel_cells=0.3)
    if name == "handover-9x22x129-b2":
        return _exotic(scenes.make_scene((9, 22, 129), seed=902, B=2, vel_cells=0.9, stick=True), 902)
    if name == "long-5x9x200":
        return scenes.make_scene((5, 9, 200), seed=903, vel_cells=2.5)
    if name == "fast-20x36x68-b2":
        return _exotic(scenes.make_scene((20, 36, 68), seed=904, B=2, vel_cells=4.0, stick=True, empty_cells=True), 904)
    if name in ("base-33x16x64", "small-half-33x16x64"):
        sc = scenes.make_scene((33, 16, 64), seed=905, vel_cells=0.9, empty_cells=True)
        if name.startswith("small"):       # half the domain flows at 1e-3 of the other scene's velocity
            sc["U"][..., :32] *= np.float32(1e-3)
        return sc
    if name == "rough-9x22x129":
        return scenes.rough_scene((9, 22, 129), seed=906, obstacle_frac=0.1, empty_frac=0.05)
    if name == "bigdt-7x13x70-b2":
        return scenes.make_scene((7, 13, 70), seed=907, B=2, vel_cells=0.9, dt=0.4, stick=True)
    raise KeyError(name)


SCENES = ["slow-7x13x70", "handover-9x22x129-b2", "long-5x9x200", "fast-20x36x68-b2", "base-33x16x64", "small-half-33x16x64",
          "rough-9x22x129", "bigdt-7x13x70-b2"]
CASES = [("advectVel", "eulerOurs"), ("advectVel", "maccormackOurs"), ("advectScalar", "eulerOurs"), ("advectScalar", "maccormackOurs")]
STRENGTH = 0.6


def evaluate(oracle, sc, op, method, mode):
    if op == "advectVel":
        return advect_vel(oracle, sc["dt"], sc["U"], sc["flags"], method, STRENGTH, mode)
    return advect_scalar(oracle, sc["dt"], sc["density"], sc["U"], sc["flags"], method, STRENGTH, mode)


def run_op(tf, sc, op, method):
    """the operator through `tf` (oracle / HIP adapter)"""
    if op == "advectVel":
        a = sc["U"].copy()
        tf.advectVel(sc["dt"], a, sc["flags"], method, None, STRENGTH)
    else:
        a = sc["density"].copy()
        tf.advectScalar(sc["dt"], a, sc["U"], sc["flags"], method, None, False, STRENGTH)
    return a
