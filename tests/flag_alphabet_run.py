"""Helper of tests/test_hip_flag_alphabet.py: own process, because the kernel-form switches (TFL_VORT_FUSED / TFL_VORT_PIPE,
TFL_VEL3_KZ / TFL_SCAL3_TZ / TFL_SCAL3_MARCH / TFL_ADV_PAIR, TFL_JACOBI_LDS) are read once per process. Every mode holds the
device result to the C oracle bit for bit on the flag-alphabet scenes (tests/flag_alphabet.py) and prints one line
`FLAG_ALPHABET_OK <mode> words=<compared> mismatches=0`.
  vort    vorticityConfinement in place and with USrc= on every 3-D and 2-D case
  advect  advectScalar / advectVel, all six methods, exact mode, on the 3-D cases
  jacobi  solveLinearSystemJacobi on the square 2-D grids LDS_GRIDS, all within jacobi.hip's one-launch LDS solve (1024 threads):
          30 x 30 = 900 cells (k_jacobi_lds<1>), 34 x 34 = 1156 and 64 x 64 = 4096 (<4>), 66 x 66 = 4356 (<16>); and a 3-D case
  slab    two steps with the Jacobi projection on an alphabet plume: the un-cut native step against oracle/simulate_np, and
          virtual z-slab ranks (world 2 and 3, uneven cuts) against the un-cut step"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import flag_alphabet as FA  # noqa: E402

LDS_GRIDS = [(1, 30, 30), (1, 34, 34), (1, 64, 64), (1, 66, 66)]


def vort(hip, ora):
    import torch
    from fluidnet_amd import tfluids
    words = 0
    for kind, dims, border in FA.CASES:
        sc = FA.scene(kind, dims, border)
        want = sc["U"].copy()
        ora.vorticityConfinement(want, sc["flags"], 0.7)
        U, fl = torch.from_numpy(sc["U"]).to(hip.dev), torch.from_numpy(sc["flags"]).to(hip.dev)
        a = U.clone()
        tfluids.vorticityConfinement(a, fl, 0.7)
        b = torch.full_like(U, float("nan"))
        tfluids.vorticityConfinement(b, fl, 0.7, USrc=U)
        for name, t in (("in place", a), ("USrc", b)):
            got = t.cpu().numpy()
            assert np.array_equal(got, want), (FA.case_id(kind, dims, border), name, int((got != want).sum()))
            words += got.size
    return words


def advect(hip, ora):
    from golden.make_golden import METHODS
    words = 0
    for kind, dims, border in FA.CASES:
        if dims[0] == 1:
            continue
        sc = FA.scene(kind, dims, border)
        gh, go = FA.Guard(hip), FA.Guard(ora)
        for m in METHODS:
            a, b = sc["density"].copy(), sc["density"].copy()
            gh.advectScalar(sc["dt"], a, sc["U"].copy(), sc["flags"], m, maccormackStrength=0.75)
            go.advectScalar(sc["dt"], b, sc["U"].copy(), sc["flags"], m, maccormackStrength=0.75)
            ua, ub = sc["U"].copy(), sc["U"].copy()
            gh.advectVel(sc["dt"], ua, sc["flags"], m, maccormackStrength=0.6)
            go.advectVel(sc["dt"], ub, sc["flags"], m, maccormackStrength=0.6)
            assert gh.raised == go.raised, (FA.case_id(kind, dims, border), m, sorted(gh.raised ^ go.raised))
            for key, x, y in (("advectScalar_" + m, a, b), ("advectVel_" + m, ua, ub)):
                if key in go.raised:
                    continue
                assert np.array_equal(x, y), (FA.case_id(kind, dims, border), key, int((x != y).sum()))
                words += x.size
    return words


def jacobi_cases():
    return [(k, g, b) for g in LDS_GRIDS for k, b in FA.KINDS] + [("alphabet", (5, 9, 21), True)]


def jacobi(hip, ora):
    words = 0
    for kind, dims, border in jacobi_cases():
        sc = FA.scene(kind, dims, border)
        f, U = sc["flags"], sc["U"].copy()
        ora.setWallBcsForward(U, f)
        div = np.zeros_like(sc["p"])
        ora.velocityDivergenceForward(U, f, div)
        for iters in (1, 2, 7, 20):
            pa, pb = np.full_like(div, 3.0), np.full_like(div, -1.0)
            ra = ora.solveLinearSystemJacobi(pa, f, div, sc["is3d"], 0.0, iters)
            rb = hip.solveLinearSystemJacobi(pb, f, div, sc["is3d"], 0.0, iters)
            assert np.array_equal(pa, pb), (FA.case_id(kind, dims, border), iters, int((pa != pb).sum()))
            assert abs(ra - rb) <= 1e-5 * max(abs(ra), 1e-30), (ra, rb)
            words += pa.size
    return words


def slab(hip, ora):
    import torch
    import scenes
    import test_hip_simulate as T
    import test_hip_slab_jacobi as J
    import test_hip_slab_methods as M
    from fluidnet_amd.dist import run_virtual_ranks
    from fluidnet_amd.simulate import simulate_native
    from oracle import simulate_np as S
    words = 0
    conf = M.mconf("maccormackOurs")
    for world in (2, 3):
        nb = FA.plume(9 * world + 4, scenes.ALPHABET, 5 + world)
        tb, tc = T._to_dev(nb, hip.dev), T._to_dev(nb, hip.dev)
        sims = J.slab_sims(tc, conf, J.uneven_cuts(nb["flags"].shape[2], world))
        for _ in range(2):
            S.simulate(ora, conf, nb, None)
            simulate_native(None, conf, tb, None)
        run_virtual_ranks(sims, 2)
        for k in ("pDiv", "UDiv", "density"):
            got = tb[k].cpu().numpy()
            assert np.array_equal(got, nb[k]), (world, k, int((got != nb[k]).sum()))
            words += 2 * got.size
        J.assert_owned_equal(sims, tb)
        for s_ in sims:
            s_.close()
    return words


if __name__ == "__main__":
    from hip_adapter import HipTfluids
    from oracle.oracle import OracleTfluids
    mode = sys.argv[1]
    n = {"vort": vort, "advect": advect, "jacobi": jacobi, "slab": slab}[mode](HipTfluids(), OracleTfluids())
    print("FLAG_ALPHABET_OK %s words=%d mismatches=0" % (mode, n))
