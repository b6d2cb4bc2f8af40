"""The mixed batches of tests/test_hip_pcg_batched.py (solveLinearSystemPCGBatched, fluidnet_amd/csrc/pcg_batched.inc): every
item is a scenes.pcg_problem of its own, with its own flags, so that the items of one batch differ in everything the batched
schedule has to keep apart -- the number of components (rounds in which some items have no system), closed and open components
(which kernels of the multigrid cycle run), components of one cell (skipped) and of fewer than five (unpreconditioned), and the
iterations to convergence (items that are done while others go on). tests/test_pcg_batched_cases_cpu.py holds the batches to
those conditions with the fp64 restatement; a batch that met none of them could not show a batched solve that mixes items up."""
import functools

import numpy as np

import pcg_ref64 as R

KINDS = ("box", "split", "pockets", "open")
SEED = 11
BATCHES = {"flat": (1, 24, 28), "vol": (9, 11, 13)}


def open_patch(f, dims, is3d):
    """turns the fluid cells of a patch (two rows near the top in y, all of x but three cells at either end, the middle plane in
    3-D) into empty cells, in place: their fluid neighbours get a Dirichlet condition, the component is open"""
    Z, Y, X = dims
    patch = f[:, :, (Z // 2 if is3d else 0), Y - 4:Y - 2, 3:X - 3]
    patch[patch == 1.0] = 4.0


def build_item(tf, dims, kind, seed=SEED, vel_cells=2.0):
    """(flags, U0, div, is3d) of one item: U0 is the velocity before its wall BCs, div the divergence after them.
      box      scenes.pcg_problem as it is: one closed component
      split    split=True: two large components and one of a single cell
      pockets  pcg_ref64._add_pockets: walled pockets of 2, 3 and 4 cells (each with an empty cell in its wall) and a single cell
      open     open_patch: a patch of empty cells inside the fluid: the component is open (a regular matrix)"""
    import scenes
    assert kind in KINDS
    sc, f, U, div = scenes.pcg_problem(tf, dims, seed, vel_cells=vel_cells, split=kind == "split")
    is3d = sc["is3d"]
    if kind in ("pockets", "open"):
        if kind == "pockets":
            R._add_pockets(f, is3d)
        else:
            open_patch(f, dims, is3d)
        U = sc["U"].copy()
        tf.setWallBcsForward(U, f)
        div = np.zeros_like(sc["p"])
        tf.velocityDivergenceForward(U, f, div)
    return np.ascontiguousarray(f), sc["U"].copy(), np.ascontiguousarray(div), is3d


def build_batch(tf, dims, kinds=KINDS, seed=SEED, vel_cells=2.0):
    """(flags [B, 1, Z, Y, X], U0 [B, C, Z, Y, X], div, is3d): one item per kind"""
    items = [build_item(tf, dims, k, seed, vel_cells) for k in kinds]
    f, U0, div = (np.ascontiguousarray(np.concatenate([it[i] for it in items], axis=0)) for i in range(3))
    return f, U0, div, items[0][3]


@functools.lru_cache(maxsize=None)
def batch(name, kinds=KINDS):
    """a batch of BATCHES, built once per process with the oracle's operators and shared (read-only)"""
    out = build_batch(R._oracle(), BATCHES[name], kinds)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def component_sizes(f, is3d):
    """[[size of every component in scan order] per item]"""
    return [R.label_components(f[b, 0], is3d)[1] for b in range(f.shape[0])]
