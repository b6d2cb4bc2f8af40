"""k_vort_pipe with compile-time stage sets and rotated ring slots (vorticity.hip): the results are the bits they were.

A block of the kernel marches a chunk of n planes in the steps t = za + 1 .. za + n + 5. Where n >= 4 (kPipeStatic) no step is a fill
and a drain step at once and every step is an instance with exactly its stages (the STATIC path); a shorter chunk -- the last one of
a ragged z range, or an override below 4 -- takes the step with runtime guards (the GUARDED path). Both paths index the rings by the
plane relative to the chunk. Every case runs in a child process (tests/vort_pipe_static_run.py: library and switches are chosen once
per process) and is compared BIT FOR BIT with
  * the two-launch form (TFL_VORT_FUSED=0, product library; one child for all scenes, shared), and
  * the oracle (operator scenes; as test_hip_parity.py::test_fused_vorticity_kernel_variants does).
Every word is compared as 32 bits, NaN words (sign and payload) and signed zeros included. The NaN and inf words of the "awkward"
scene sit where the operator defines every output bit (vort_pipe_static_run.py op_inputs says why and where).
The step scenes (the setConstVals pair folded into the kernel's store) have no bit-level oracle -- the projection net follows the
confinement inside the step -- and are held to the two-launch form's step. The library's entry points start a fold only from inside
a step, and the z-slab step calls the confinement under a ONE-run window; the two-run window (na and nb both non-zero) is covered at
operator level, without a fold."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vort_pipe_static_run as R  # noqa: E402
from flavours import child_env  # noqa: E402

pytestmark = pytest.mark.gpu
SWITCHES = ("TFL_VORT_PIPE", "TFL_VORT_CZ", "TFL_VORT_FUSED", "TFL_XCD_ORDER", "TFL_VORT_TILE", "TFL_BC_FOLD", "TFL_VEL3_KZ", "TFL_SCAL3_TZ")
K_STATIC = 4


def run_child(path, names, extra):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e = child_env(e, extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "vort_pipe_static_run.py"), str(path)] + list(names), env=e, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "vort pipe static ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(str(path)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def reference(tmp_path_factory, oracle):
    """every scene through the two-launch form (one child), and the operator scenes through the oracle; computed once, never changed"""
    d = tmp_path_factory.mktemp("vort_pipe_static")
    two = run_child(d / "two_launch.npz", list(R.OP_SCENES) + list(R.STEP_SCENES), {"TFL_VORT_FUSED": "0"})
    ora = {}
    for name in R.OP_SCENES:
        U, fl = R.op_inputs(name)
        oracle.vorticityConfinement(U, fl, R.STRENGTH)
        ora[name + "/full"] = U
    for v in list(two.values()) + list(ora.values()):
        v.setflags(write=False)
    return d, two, ora


def chunk_lengths(Z, cz, window=None):
    runs = [(0, Z)] if window is None else [(window[0], window[1]), (window[2], window[3])]
    return [min(cz, b - z) for a, b in runs for z in range(a, b, cz)]


def check(got, reference, names):
    _, two, ora = reference
    seen = 0
    for key in sorted(got):
        scene, what = key.split("/", 1)
        if what == "window":        # the planes of the window hold the whole-array result, the others were not written
            Z = got[key].shape[2]
            inside = np.zeros(Z, bool)
            inside[R.WINDOW[0]:R.WINDOW[1]] = True
            inside[R.WINDOW[2]:R.WINDOW[3]] = True
            refs = [("two-launch", np.where(inside[None, None, :, None, None], two[scene + "/full"], np.float32(R.OUTSIDE))),
                    ("oracle", np.where(inside[None, None, :, None, None], ora[scene + "/full"], np.float32(R.OUTSIDE)))]
        else:
            refs = [("two-launch", two[key])] + ([("oracle", ora[key])] if key in ora else [])
        for label, want in refs:
            differ = bits(got[key]) != bits(want)
            print("%s against %s: %d of %d words differ" % (key, label, int(differ.sum()), differ.size))
            assert not differ.any(), (key, label, int(differ.sum()), np.argwhere(differ)[:5].tolist())
            seen += 1
    assert seen and {k.split("/")[0] for k in got} == set(names)


@pytest.mark.parametrize("cz", [1, 3, 4, 5, 6, 7, 8, 13, 19])
def test_every_chunk_length_around_the_bound(reference, cz):
    """70 x 20 x 19 (tiles ragged in x and y), EXPERIMENTS flavour, TFL_VORT_CZ = cz: chunks below (1, 3: GUARDED), at (4) and above the
    bound (STATIC), a short last chunk behind long ones (8, 8, 3: STATIC, STATIC, GUARDED; also 5 x 3 + 4, 6 x 3 + 1, 7 + 7 + 5, 13 + 6)
    and one chunk that spans the array (19); then the same under a two-run z-window (runs of 7 and 6 planes)."""
    lens = chunk_lengths(19, cz)
    print("cz %d: chunks %s -> %s" % (cz, lens, ["STATIC" if n >= K_STATIC else "GUARDED" for n in lens]))
    print("   under the window: chunks %s" % chunk_lengths(19, cz, R.WINDOW))
    names = ["ragged19"]
    got = run_child(reference[0] / ("cz%d.npz" % cz), names, {"TFL_VORT_FUSED": "1", "TFL_VORT_CZ": str(cz)})
    assert "ragged19/window" in got
    check(got, reference, names)


def test_product_library_without_override(reference):
    """The product library, chunk length chosen by the launcher: 4 on these grids (few tiles). Z = 12 and Z = 40 are chunks of exactly
    4 planes -- AT the bound: the STATIC path with an empty steady loop --, Z = 14 ends in a chunk of 2 (GUARDED); the batch of two
    different items, the awkward words, the folded pair in the native step and in the z-slab step run here too."""
    for Z in (12, 14, 40):
        lens = chunk_lengths(Z, 4)
        print("Z %d: chunks %s -> %s" % (Z, lens, sorted({"STATIC" if n >= K_STATIC else "GUARDED" for n in lens})))
    names = ["z12", "z14", "z40", "batch2", "awkward", "fold_step", "fold_slab"]
    check(run_child(reference[0] / "product.npz", names, {"TFL_VORT_FUSED": "1"}), reference, names)


@pytest.mark.parametrize("cz", [3, 8])
def test_batch_awkward_words_and_folded_pair(reference, cz):
    """B = 2 with different fields per item; NaN, inf and -0.0 words with obstacle and empty cells on the tile edges; the setConstVals
    pair folded into the store, its box cutting every chunk boundary (native step, 20 planes) and under the z-slab step's window
    (three ranks). cz = 8: STATIC chunks with a steady loop (8, 8, 3 / 8, 8, 4); cz = 3: every chunk GUARDED."""
    names = ["batch2", "awkward", "fold_step", "fold_slab"]
    check(run_child(reference[0] / ("mixed_cz%d.npz" % cz), names, {"TFL_VORT_FUSED": "1", "TFL_VORT_CZ": str(cz)}), reference, names)


def test_tiles_of_32_by_16(reference):
    """TFL_VORT_TILE=32 (two 512-thread blocks per CU) on the 70 x 20 x 19 case and the awkward words: chunks of 4, 4, 4, 4, 3"""
    names = ["ragged19", "awkward"]
    check(run_child(reference[0] / "tile32.npz", names, {"TFL_VORT_FUSED": "1", "TFL_VORT_TILE": "32"}), reference, names)
